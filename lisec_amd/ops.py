"""Thin Python wrappers over the dense-contraction entry points of the C ABI (include/lisec_hip.h
section 3).  Tensors are torch CUDA tensors used purely as device memory."""
import bisect
import ctypes
import math

import torch

from . import _lib
from ._lib import ConvGeom
from .params import TRAINABLE_KINDS

IN_RELU, OUT_RELU, ACCUMULATE, DY_RELU, SMALL_TILE, TAG_ROOFLINE = 1, 2, 4, 8, 16, 32
# SMALL_TILE (conv_forward / conv_plan): a small K-sliced layer may run as 64-row tiles, two workgroups per CU
# (LISEC_CONV_SMALL_TILE; the plan reports tile_rows).  Same output bit for bit.


def geom(mode, in_dims, out_dims, kernel, stride, pad, cin, cout, in_stride=None, out_stride=None, ps=0,
         ps_channels=0):
    """in_dims/out_dims/kernel/stride/pad: 3-tuples (d, h, w)."""
    g = ConvGeom()
    g.mode = mode
    g.Di, g.Hi, g.Wi = in_dims
    g.Do, g.Ho, g.Wo = out_dims
    g.KD, g.KH, g.KW = kernel
    g.sd, g.sh, g.sw = stride
    g.pd, g.ph, g.pw = pad
    g.Cin, g.Cout = cin, cout
    g.in_stride = in_stride if in_stride is not None else cin
    g.out_stride = out_stride if out_stride is not None else cout
    g.ps, g.ps_channels = ps, ps_channels
    return g


def packed_floats(ntaps, K, N):
    return _lib.load().lisec_conv_packed_floats(ntaps, K, N)


def pack_weights(src, ntaps, K, N, tap_stride, k_stride, n_stride, out=None):
    """Repack a Keras-layout kernel (any strides) into the [tap][K/4][N][4] layout of the kernels."""
    lib = _lib.load()
    n = packed_floats(ntaps, K, N)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=src.device)
    assert out.numel() >= n
    _lib.check(lib.lisec_conv_pack_weights(_lib.ptr(src), ntaps, K, N, tap_stride, k_stride, n_stride,
                                           _lib.ptr(out), _lib.current_stream()))
    return out


class PackTable:
    """Device-resident table for lisec_conv_pack_weights_batched: entries (src, dst, ntaps, K, N, strides)."""

    def __init__(self, entries, device):
        arr = (_lib.PackDesc * len(entries))()
        start = 0
        for d, (src, dst, ntaps, K, N, ts, ks, ns) in zip(arr, entries):
            Kp, Np = (K + 63) // 64 * 64, (N + 63) // 64 * 64
            d.src, d.dst = src.data_ptr(), dst.data_ptr()
            d.tap_stride, d.k_stride, d.n_stride, d.start = ts, ks, ns, start
            d.ntaps, d.K, d.N, d.Kp, d.Np = ntaps, K, N, Kp, Np
            assert dst.numel() >= ntaps * Kp * Np
            start += ntaps * Kp * Np
        self.total, self.n = start, len(entries)
        self.keep = [e[0] for e in entries] + [e[1] for e in entries]
        raw = bytes(arr)
        self.table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)

    def run(self):
        _lib.check(_lib.load().lisec_conv_pack_weights_batched(_lib.ptr(self.table), self.n, self.total,
                                                               _lib.current_stream()))


class CopyTable:
    """Device-resident table for lisec_copy2d_batched: entries (src, dst) of equal 1-D / 2-D shapes (views allowed)."""

    def __init__(self, pairs, device):
        arr = (_lib.CopyDesc * len(pairs))()
        for d, (src, dst) in zip(arr, pairs):
            assert src.shape == dst.shape and src.dim() in (1, 2) and src.dtype == dst.dtype == torch.float32
            rows, cols = (1, src.shape[0]) if src.dim() == 1 else src.shape
            assert src.stride(-1) == 1 and dst.stride(-1) == 1
            d.src, d.dst, d.rows, d.cols = src.data_ptr(), dst.data_ptr(), rows, cols
            d.src_stride = src.stride(0) if src.dim() == 2 else cols
            d.dst_stride = dst.stride(0) if dst.dim() == 2 else cols
        self.n, self.keep = len(pairs), pairs
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)

    def run(self):
        _lib.check(_lib.load().lisec_copy2d_batched(_lib.ptr(self.table), self.n, _lib.current_stream()))


def num_mblocks(g):
    n = _lib.load().lisec_conv_num_mblocks(ctypes.byref(g))
    if n < 0:
        raise _lib.LisecError(_lib.load().lisec_last_error().decode())
    return n


_SPLITK_WS = {}


def conv_workspace(g, device, row_capacity=0, tag="main"):
    """Shared split-K scratch for `g` (None when the layer is large enough to run in one pass); one buffer per stream
    role (tag): contractions that may run at the same time on two streams must not share their slabs.  Zero-filled:
    it starts with the arrival counters of the K slices, which every call leaves at zero (include/lisec_hip.h)."""
    lib = _lib.load()
    need = (lib.lisec_conv_forward_rows_workspace_bytes(ctypes.byref(g), row_capacity) if row_capacity > 0
            else lib.lisec_conv_forward_workspace_bytes(ctypes.byref(g)))
    if need == 0:
        return None
    key = (str(device), tag)
    if key not in _SPLITK_WS or _SPLITK_WS[key].numel() < need:
        if key in _SPLITK_WS:
            torch.cuda.synchronize(device)          # a call on another stream may still be using the old buffer
        _SPLITK_WS[key] = torch.zeros(need, dtype=torch.uint8, device=device)
        _lib.bump_alloc_generation()                # recorded step plans hold the old address
    return _SPLITK_WS[key]


class BnSink:
    """lisec_bn_sink: the per-tile BatchNormalization sums of a contraction go into fixed-point accumulators and the
    last workgroup of the call finalises them (no stats table, no finaliser launch).  Forward: bnstate (+ moving
    statistics); backward: dgamma / dbeta / coef (feed bn_backward_apply_coef)."""

    def __init__(self, C, n_rows, device, gamma=None, beta=None, moving_mean=None, moving_var=None, unbiased=True,
                 bnstate=None, dgamma=None, dbeta=None):
        lib = _lib.load()
        self.acc = torch.zeros(lib.lisec_bn_sink_words(C), dtype=torch.int64, device=device)    # zero before first use
        self.backward = dgamma is not None
        self.coef = torch.zeros(2 * C, dtype=torch.float32, device=device) if self.backward else None
        self.keep = (gamma, beta, moving_mean, moving_var, bnstate, dgamma, dbeta)
        d = _lib.BnSinkDesc()
        d.acc, d.kind, d.unbiased_moving, d.n_rows = self.acc.data_ptr(), 2 if self.backward else 1, 1 if unbiased else 0, float(n_rows)
        d.gamma, d.beta = _lib.ptr(gamma), _lib.ptr(beta)
        d.moving_mean, d.moving_var, d.bnstate = _lib.ptr(moving_mean), _lib.ptr(moving_var), _lib.ptr(bnstate)
        d.dgamma, d.dbeta, d.coef = _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(self.coef)
        self.desc = d
        self.ref = ctypes.pointer(d)


def _fold_fields(fold):
    if fold is None:
        return None, None, None, 0
    return _lib.ptr(fold[0]), _lib.ptr(fold[1]), _lib.ptr(fold[2]), 1 if fold[3] else 0


def conv_forward(g, x, wp, out, bias=None, in_bn=None, flags=0, stats=None, splitk=True, rows=None, out_mask=None,
                 bwd=None, sink=None, ws_tag="main", queue=None, tail=None, fold=None, dense_dw=None, workspace=None):
    """rows: optional (row_coords int32 (cap,3), row_count int32 device scalar, capacity) row list.
    out_mask: optional tensor laid out like `out`; values are stored as 0 where out_mask <= 0.
    bwd: optional (y, bnstate, relu): `out` is a gradient about to cross that BatchNormalization(+ReLU) backwards and
    `stats` (num_mblocks_bwd(g) rows) receives the per-tile (sum dz, sum dz*yhat) -- see bn_backward_apply.
    sink: optional BnSink taking the per-tile sums instead of `stats` (finalised inside the call).
    queue: optional int32[2] device tensor, zero before its first use: lets a big row list run as resident workgroups
    that draw their tiles from a counter (lisec_conv_extras.queue).
    tail: optional (packed 64 x 64 kernel, out2): out2 = out (as stored) @ kernel rides on the tile; bwd / sink then describe
    out2 (lisec_conv_extras.tail_w).
    fold: optional (y, bnstate, coef, relu): x is a gradient about to cross that BatchNormalization(+ReLU) backwards and the
    apply pass runs on load (lisec_conv_extras.in_y).
    dense_dw: optional float32 tensor of dense_dw_slabs() * 4096 elements: the call is a Dense(64)'s data gradient (bwd + sink)
    and also leaves the per-workgroup slabs of the Dense's weight gradient there (lisec_conv_extras.dense_dw; dense_dw_reduce).
    workspace: optional uint8 tensor the call uses as its split-K scratch instead of the shared conv_workspace() buffer; its
    head (the arrival counters) must be zero, and the plan is made for its size."""
    rc, rn, cap = rows if rows is not None else (None, None, 0)
    if workspace is not None:
        ws = workspace
    else:
        ws = conv_workspace(g, out.device, cap, ws_tag) if splitk else None
    ex = _lib.ConvExtras(_lib.ptr(out_mask), _lib.ptr(bwd[0]) if bwd is not None else None,
                         _lib.ptr(bwd[1]) if bwd is not None else None, 1 if (bwd is not None and bwd[2]) else 0,
                         sink.ref if sink is not None else None, _lib.ptr(queue),
                         _lib.ptr(tail[0]) if tail is not None else None, _lib.ptr(tail[1]) if tail is not None else None,
                         *_fold_fields(fold), _lib.ptr(dense_dw))
    _lib.check(_lib.load().lisec_conv_forward_ex(ctypes.byref(g), _lib.ptr(x), _lib.ptr(wp), _lib.ptr(bias),
                                                 _lib.ptr(in_bn), flags, _lib.ptr(out), ctypes.byref(ex),
                                                 _lib.ptr(stats), _lib.ptr(ws),
                                                 ws.numel() if ws is not None else 0,
                                                 _lib.ptr(rc), _lib.ptr(rn), cap, _lib.current_stream()))
    return out


def packed_bf16_bytes(ntaps, K, N):
    return _lib.load().lisec_conv_packed_bf16_bytes(ntaps, K, N)


def pack_weights_bf16(src, ntaps, K, N, tap_stride, k_stride, n_stride, out=None):
    """Round a Keras-layout fp32 kernel (any strides) to bf16, nearest-even, into the [tap][K/8][N][8] layout of the bf16
    inference kernel (lisec_conv_pack_weights_bf16); out: uint8 tensor of packed_bf16_bytes(ntaps, K, N)."""
    n = packed_bf16_bytes(ntaps, K, N)
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=src.device)
    assert out.numel() >= n
    _lib.check(_lib.load().lisec_conv_pack_weights_bf16(_lib.ptr(src), ntaps, K, N, tap_stride, k_stride, n_stride,
                                                        _lib.ptr(out), _lib.current_stream()))
    return out


def conv_bf16_workspace(g, device, tag="main"):
    """The split-K scratch of conv_workspace (same buffers, same zero-counter contract), sized for the bf16 kernel's plan."""
    need = _lib.load().lisec_conv_forward_bf16_workspace_bytes(ctypes.byref(g))
    if need == 0:
        return None
    key = (str(device), tag)
    if key not in _SPLITK_WS or _SPLITK_WS[key].numel() < need:
        if key in _SPLITK_WS:
            torch.cuda.synchronize(device)
        _SPLITK_WS[key] = torch.zeros(need, dtype=torch.uint8, device=device)
        _lib.bump_alloc_generation()
    return _SPLITK_WS[key]


def conv_forward_bf16(g, x, wp, out, bias=None, in_bn=None, flags=0, splitk=True, ws_tag="main"):
    """conv_forward(...) with bf16 MFMA operands (lisec_conv_forward_bf16): fp32 x / out / bias / in_bn, wp from
    pack_weights_bf16.  Forward geometries only; anything the kernel does not serve raises LisecError."""
    ws = conv_bf16_workspace(g, out.device, ws_tag) if splitk else None
    _lib.check(_lib.load().lisec_conv_forward_bf16(ctypes.byref(g), _lib.ptr(x), _lib.ptr(wp), _lib.ptr(out),
                                                   _lib.ptr(bias), _lib.ptr(in_bn), flags, _lib.ptr(ws),
                                                   ws.numel() if ws is not None else 0, _lib.current_stream()))
    return out


def dense_dw_slabs():
    """Slabs (of 64 x 64 floats) a conv_forward(..., dense_dw=) call writes (lisec_dense_dw_slabs)."""
    return _lib.load().lisec_dense_dw_slabs()


def dense_dw_reduce(slabs, dW):
    """dW (64, 64) = the slabs of a conv_forward(..., dense_dw=slabs) call summed in index order (lisec_dense_dw_reduce)."""
    _lib.check(_lib.load().lisec_dense_dw_reduce(_lib.ptr(slabs), _lib.ptr(dW), _lib.current_stream()))
    return dW


def winograd_packed_floats(KD, K, N):
    return _lib.load().lisec_conv_winograd_packed_floats(KD, K, N)


def pack_weights_winograd(src, KD, K, N, tap_stride, k_stride, n_stride, flip=False, out=None):
    """G g G^T of a (KD, 3, 3, ...) kernel in the Winograd kernel's LDS image order (lisec_conv_pack_weights_winograd);
    flip mirrors the (kh, kw) taps: the kernel a data gradient (mode 1) takes."""
    n = winograd_packed_floats(KD, K, N)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=src.device)
    assert out.numel() >= n
    _lib.check(_lib.load().lisec_conv_pack_weights_winograd(_lib.ptr(src), KD, K, N, tap_stride, k_stride, n_stride,
                                                            1 if flip else 0, _lib.ptr(out), _lib.current_stream()))
    return out


def _wino_extras(out_mask, bwd, sink, tail=None):
    return _lib.ConvExtras(_lib.ptr(out_mask), _lib.ptr(bwd[0]) if bwd is not None else None,
                           _lib.ptr(bwd[1]) if bwd is not None else None, 1 if (bwd is not None and bwd[2]) else 0,
                           sink.ref if sink is not None else None, None,
                           _lib.ptr(tail[0]) if tail is not None else None, _lib.ptr(tail[1]) if tail is not None else None,
                           None, None, None, 0)


def winograd_supported(g, in_bn=False, flags=0, out_mask=None, bwd=None, sink=None, tail=None):
    ex = _wino_extras(out_mask, bwd, sink, tail)
    return bool(_lib.load().lisec_conv_winograd_supported(ctypes.byref(g), 1 if in_bn else 0, flags, ctypes.byref(ex)))


def conv_forward_winograd(g, x, wu, out, bias=None, in_bn=None, flags=0, out_mask=None, bwd=None, sink=None, tail=None):
    """conv_forward(...) in the Winograd F(2x2, 3x3) form (lisec_conv_forward_winograd); wu from pack_weights_winograd.
    tail: optional (packed 64 x 64 kernel, out2) as in conv_forward: out2 = out (as stored) @ kernel; bwd / sink describe out2."""
    ex = _wino_extras(out_mask, bwd, sink, tail)
    _lib.check(_lib.load().lisec_conv_forward_winograd(ctypes.byref(g), _lib.ptr(x), _lib.ptr(wu), _lib.ptr(bias),
                                                       _lib.ptr(in_bn), flags, _lib.ptr(out), ctypes.byref(ex),
                                                       _lib.current_stream()))
    return out


def conv_plan(g, in_bn=False, flags=0, stats=False, splitk=True, rows_capacity=0, out_mask=None, bwd=None, sink=None,
              queue=None, tail=None, fold=None, dense_dw=None):
    """The launch plan conv_forward(...) with the same arguments runs (lisec_conv_plan_query), as a dict."""
    lib = _lib.load()
    ws_bytes = 0
    if splitk:
        ws_bytes = (lib.lisec_conv_forward_rows_workspace_bytes(ctypes.byref(g), rows_capacity) if rows_capacity > 0
                    else lib.lisec_conv_forward_workspace_bytes(ctypes.byref(g)))
    ex = _lib.ConvExtras(_lib.ptr(out_mask), _lib.ptr(bwd[0]) if bwd is not None else None,
                         _lib.ptr(bwd[1]) if bwd is not None else None, 1 if (bwd is not None and bwd[2]) else 0,
                         sink.ref if sink is not None else None, _lib.ptr(queue),
                         _lib.ptr(tail[0]) if tail is not None else None, _lib.ptr(tail[1]) if tail is not None else None,
                         *_fold_fields(fold), _lib.ptr(dense_dw))
    plan = _lib.ConvPlan()
    _lib.check(lib.lisec_conv_plan_query(ctypes.byref(g), 1 if in_bn else 0, flags, ctypes.byref(ex), 1 if stats else 0,
                                         ws_bytes, 1 if rows_capacity > 0 else 0, rows_capacity, ctypes.byref(plan)))
    d = {n: getattr(plan, n) for n, _ in _lib.ConvPlan._fields_}
    d["kernel"] = _lib.KERNEL_NAMES[d["kernel"]]
    return d


def num_mblocks_bwd(g):
    n = _lib.load().lisec_conv_num_mblocks_bwd(ctypes.byref(g))
    if n < 0:
        raise _lib.LisecError(_lib.load().lisec_last_error().decode())
    return n


def bn_backward_apply(dA, da_stride, y, bnstate, M, C, relu, parts, nparts, dgamma, dbeta, dy):
    """Passes 2-3 of bn_backward on partials written by conv_forward(..., bwd=...)."""
    ws = _ew_workspace(y.device)
    _lib.check(_lib.load().lisec_bn_backward_apply(_lib.ptr(dA), da_stride, _lib.ptr(y), _lib.ptr(bnstate), M, C,
                                                   1 if relu else 0, _lib.ptr(parts), nparts, _lib.ptr(dgamma),
                                                   _lib.ptr(dbeta), _lib.ptr(dy), _lib.ptr(ws), ws.numel(),
                                                   _lib.current_stream()))


def bn_backward_apply_coef(dA, da_stride, y, bnstate, M, C, relu, coef, dy):
    """The apply pass alone, with the coefficients a backward BnSink produced."""
    _lib.check(_lib.load().lisec_bn_backward_apply_coef(_lib.ptr(dA), da_stride, _lib.ptr(y), _lib.ptr(bnstate), M, C,
                                                        1 if relu else 0, _lib.ptr(coef), _lib.ptr(dy),
                                                        _lib.current_stream()))


def bn_finalize(partials, nparts, C, n_rows, gamma, beta, moving_mean, moving_var, unbiased, bnstate):
    _lib.check(_lib.load().lisec_bn_finalize(_lib.ptr(partials), nparts, C, float(n_rows), _lib.ptr(gamma),
                                             _lib.ptr(beta), _lib.ptr(moving_mean), _lib.ptr(moving_var),
                                             1 if unbiased else 0, _lib.ptr(bnstate), _lib.current_stream()))


def bn_fold(gamma, beta, moving_mean, moving_var, C, bnstate):
    _lib.check(_lib.load().lisec_bn_fold(_lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(moving_mean),
                                         _lib.ptr(moving_var), C, _lib.ptr(bnstate), _lib.current_stream()))


def wgrad_workspace_bytes(g, row_capacity=0):
    return _lib.load().lisec_conv_wgrad_workspace_bytes(ctypes.byref(g), row_capacity)


def wgrad_plan(g, flags=0, dy_bn=False, rows_capacity=0):
    """The launch plan conv_wgrad(...) runs for these arguments (lisec_conv_wgrad_plan_query), as a dict."""
    plan = _lib.WgradPlan()
    _lib.check(_lib.load().lisec_conv_wgrad_plan_query(ctypes.byref(g), flags, 1 if dy_bn else 0,
                                                       1 if rows_capacity > 0 else 0, rows_capacity, ctypes.byref(plan)))
    return {n: getattr(plan, n) for n, _ in _lib.WgradPlan._fields_}


class WgradBatch:
    """lisec_conv_wgrad_batched over fixed tensors: items = [(geom, x, dy, dW, in_bn or None, flags, transpose_out), ...]
    (at most 6).  The stride-1 convolutions of one RPN block share one launch."""

    def __init__(self, items):
        self.n = len(items)
        self.keep = items
        self.arr = (_lib.WgradItem * self.n)()
        for a, (g, x, dy, dW, in_bn, flags, transpose_out) in zip(self.arr, items):
            a.g = ctypes.pointer(g)
            a.in_, a.in_bnstate, a.flags = x.data_ptr(), _lib.ptr(in_bn), flags
            a.dy, a.transpose_out, a.dW = dy.data_ptr(), 1 if transpose_out else 0, dW.data_ptr()

    def workspace_bytes(self):
        return _lib.load().lisec_conv_wgrad_batched_workspace_bytes(self.arr, self.n)

    def run(self, workspace):
        _lib.check(_lib.load().lisec_conv_wgrad_batched(self.arr, self.n, _lib.ptr(workspace),
                                                        workspace.numel() * workspace.element_size(),
                                                        _lib.current_stream()))


def conv_wgrad(g, x, dy, dW, workspace, in_bn=None, flags=0, transpose_out=False, dy_bn=None, rows=None):
    rc, rn, cap = rows if rows is not None else (None, None, 0)
    _lib.check(_lib.load().lisec_conv_wgrad(ctypes.byref(g), _lib.ptr(x), _lib.ptr(in_bn), flags, _lib.ptr(dy),
                                            _lib.ptr(dy_bn), _lib.ptr(workspace),
                                            workspace.numel() * workspace.element_size(),
                                            1 if transpose_out else 0, _lib.ptr(dW), _lib.ptr(rc), _lib.ptr(rn), cap,
                                            _lib.current_stream()))
    return dW


def wgrad_winograd_supported(g):
    return bool(_lib.load().lisec_conv_wgrad_winograd_supported(ctypes.byref(g)))


def wgrad_winograd_workspace_bytes(g):
    return _lib.load().lisec_conv_wgrad_winograd_workspace_bytes(ctypes.byref(g))


def conv_wgrad_winograd(g, x, dy, dW, workspace):
    """conv_wgrad(g, x, dy, dW, ...) in the Winograd F(2x2, 3x3) form (lisec_conv_wgrad_winograd): 64 -> 64 Conv3D blocks."""
    _lib.check(_lib.load().lisec_conv_wgrad_winograd(ctypes.byref(g), _lib.ptr(x), _lib.ptr(dy), _lib.ptr(workspace),
                                                     workspace.numel() * workspace.element_size(), _lib.ptr(dW),
                                                     _lib.current_stream()))
    return dW


_EW = {}


def _ew_workspace(device, tag="main"):
    """Scratch of the element-wise entry points; launches that may run at the same time on different streams must not
    share one (tag: one buffer per stream role)."""
    key = (str(device), tag)
    if key not in _EW:
        _EW[key] = torch.empty(_lib.load().lisec_eltwise_workspace_bytes(), dtype=torch.uint8, device=device)
    return _EW[key]


def bn_backward(dA, da_stride, y, bnstate, M, C, relu, dgamma, dbeta, dy, dbias=None):
    ws = _ew_workspace(y.device)
    _lib.check(_lib.load().lisec_bn_backward(_lib.ptr(dA), da_stride, _lib.ptr(y), _lib.ptr(bnstate), M, C,
                                             1 if relu else 0, _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(dbias),
                                             _lib.ptr(dy), _lib.ptr(ws), ws.numel(), _lib.current_stream()))


def relu_mask(grad, act):
    _lib.check(_lib.load().lisec_relu_mask(_lib.ptr(grad), _lib.ptr(act), grad.numel(), _lib.current_stream()))


def colsum(x, stride, M, C, out, ws_tag="main"):
    ws = _ew_workspace(x.device, ws_tag)
    _lib.check(_lib.load().lisec_colsum(_lib.ptr(x), stride, M, C, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                        _lib.current_stream()))


def rpn_loss(head, y_cls, y_reg, M, kind, dhead, loss_out, grad_scale=1.0):
    ws = _ew_workspace(head.device)
    _lib.check(_lib.load().lisec_rpn_loss(_lib.ptr(head), _lib.ptr(y_cls), _lib.ptr(y_reg), M, kind, grad_scale,
                                          _lib.ptr(dhead), _lib.ptr(loss_out), _lib.ptr(ws), ws.numel(),
                                          _lib.current_stream()))


def rpn_loss_eval(head, y_cls, y_reg, M, kind, acc):
    """Adds the [total, class, regression] that rpn_loss would write to loss_out (the same fp32 bits) to acc[0:3] and
    counts the sweep in acc[3] (acc: float64[4] device tensor); no gradient."""
    ws = _ew_workspace(head.device)
    _lib.check(_lib.load().lisec_rpn_loss_eval(_lib.ptr(head), _lib.ptr(y_cls), _lib.ptr(y_reg), M, kind, _lib.ptr(acc),
                                               _lib.ptr(ws), ws.numel(), _lib.current_stream()))


def _loss_workspace(device):
    ws = _ew_workspace(device)
    assert ws.numel() >= _lib.load().lisec_head_loss_workspace_bytes()
    return ws


def head_loss(cfg, head, y_cls, y_reg, M, dhead, loss_out, metric_out=None, grad_scale=1.0):
    """The Keras losses / metrics of cfg (an _lib.LossCfg, lisec_loss_cfg): dhead, loss_out = [total, class, regression]
    and metric_out (float32 device tensor, one value per metric: the class output's, then the regression output's)."""
    ws = _loss_workspace(head.device)
    _lib.check(_lib.load().lisec_head_loss(ctypes.byref(cfg), _lib.ptr(head), _lib.ptr(y_cls), _lib.ptr(y_reg), M,
                                           grad_scale, _lib.ptr(dhead), _lib.ptr(loss_out), _lib.ptr(metric_out),
                                           _lib.ptr(ws), ws.numel(), _lib.current_stream()))


def head_loss_eval(cfg, head, y_cls, y_reg, M, acc):
    """Adds the values head_loss would write -- [total, class, regression, metrics...], the same fp32 bits -- to acc
    (float64 device tensor of 4 + number of metrics) and counts the sweep in its last word; no gradient."""
    ws = _loss_workspace(head.device)
    _lib.check(_lib.load().lisec_head_loss_eval(ctypes.byref(cfg), _lib.ptr(head), _lib.ptr(y_cls), _lib.ptr(y_reg), M,
                                                _lib.ptr(acc), _lib.ptr(ws), ws.numel(), _lib.current_stream()))


def _detection_workspace(device):
    ws = _ew_workspace(device)
    assert ws.numel() >= _lib.load().lisec_detection_loss_workspace_bytes()
    return ws


def detection_loss(cfg, head, y_cls, y_reg, M, dhead, loss_out, counts_out, grad_scale=1.0):
    """The VoxelNet detection loss of cfg (an _lib.DetectionLossCfg, lisec_detection_loss_cfg): dhead, loss_out = [total,
    class, regression] and counts_out = [N_pos, N_neg] (int64 device tensor)."""
    ws = _detection_workspace(head.device)
    _lib.check(_lib.load().lisec_detection_loss(ctypes.byref(cfg), _lib.ptr(head), _lib.ptr(y_cls), _lib.ptr(y_reg), M,
                                                grad_scale, _lib.ptr(dhead), _lib.ptr(loss_out), _lib.ptr(counts_out),
                                                _lib.ptr(ws), ws.numel(), _lib.current_stream()))


def detection_loss_eval(cfg, head, y_cls, y_reg, M, acc):
    """Adds the [total, class, regression] detection_loss would write (the same fp32 bits) to acc[0:3] and counts the
    sweep in acc[3] (float64[4] device tensor); no gradient."""
    ws = _detection_workspace(head.device)
    _lib.check(_lib.load().lisec_detection_loss_eval(ctypes.byref(cfg), _lib.ptr(head), _lib.ptr(y_cls), _lib.ptr(y_reg),
                                                     M, _lib.ptr(acc), _lib.ptr(ws), ws.numel(), _lib.current_stream()))


def detection_iou_loss(cfg, head, y_cls, y_reg, M, dhead, loss_out, counts_out, grad_scale=1.0):
    """The detection loss with the IoU term of cfg (an _lib.DetectionIoULossCfg, lisec_detection_iou_loss_cfg): the
    outputs of detection_loss, the IoU term inside the regression value and gradient."""
    ws = _ew_workspace(head.device)
    assert ws.numel() >= _lib.load().lisec_detection_iou_loss_workspace_bytes()
    _lib.check(_lib.load().lisec_detection_iou_loss(ctypes.byref(cfg), _lib.ptr(head), _lib.ptr(y_cls), _lib.ptr(y_reg), M,
                                                    grad_scale, _lib.ptr(dhead), _lib.ptr(loss_out),
                                                    _lib.ptr(counts_out), _lib.ptr(ws), ws.numel(),
                                                    _lib.current_stream()))


def detection_iou_loss_eval(cfg, head, y_cls, y_reg, M, acc):
    """Adds the [total, class, regression] detection_iou_loss would write (the same fp32 bits) to acc[0:3] and counts the
    sweep in acc[3] (float64[4] device tensor); no gradient."""
    ws = _ew_workspace(head.device)
    assert ws.numel() >= _lib.load().lisec_detection_iou_loss_workspace_bytes()
    _lib.check(_lib.load().lisec_detection_iou_loss_eval(ctypes.byref(cfg), _lib.ptr(head), _lib.ptr(y_cls),
                                                         _lib.ptr(y_reg), M, _lib.ptr(acc), _lib.ptr(ws), ws.numel(),
                                                         _lib.current_stream()))


def sample_weights(w_cls, w_reg, M, weighted_metrics=(0, 0), per_cell=None):
    """The lisec_sample_weights (an _lib.SampleWeights) of one weight tensor per output (float32, device; None: that
    output has weight 1): one element is the sweep's weight, more are the map over the M cells.  per_cell overrides the
    form read from the sizes (a value outside {0, 1} is the library's to refuse).  The descriptor holds addresses: the caller keeps the tensors alive, and a recorded plan
    reads whatever they hold when it is replayed.  weighted_metrics: per output, bit j = metric j is weighted."""
    sw = _lib.SampleWeights()
    sw.struct_bytes = ctypes.sizeof(_lib.SampleWeights)
    for o, w in enumerate((w_cls, w_reg)):
        if w is not None:
            assert w.dtype == torch.float32 and w.is_contiguous()
        sw.per_cell[o] = int(per_cell[o]) if per_cell is not None else int(w is not None and w.numel() > 1)
        if w is not None and sw.per_cell[o] == 1 and w.numel() < M:
            raise ValueError(f"a weight map of {w.numel()} cells for a grid of {M}")
        sw.w[o] = _lib.ptr(w)
        sw.weighted_metrics[o] = int(weighted_metrics[o])
    return sw


def head_loss_weighted(cfg, sw, head, y_cls, y_reg, M, dhead, loss_out, metric_pairs=None, grad_scale=1.0):
    """head_loss under the sample weights sw (sample_weights()): dhead, loss_out, and metric_pairs (float64 device tensor)
    = [num0, den0, num1, den1, ...], one pair per metric of cfg."""
    ws = _ew_workspace(head.device)
    assert ws.numel() >= _lib.load().lisec_head_loss_weighted_workspace_bytes()
    _lib.check(_lib.load().lisec_head_loss_weighted(ctypes.byref(cfg), ctypes.byref(sw), _lib.ptr(head), _lib.ptr(y_cls),
                                                    _lib.ptr(y_reg), M, grad_scale, _lib.ptr(dhead), _lib.ptr(loss_out),
                                                    _lib.ptr(metric_pairs), _lib.ptr(ws), ws.numel(),
                                                    _lib.current_stream()))


def head_loss_weighted_eval(cfg, sw, head, y_cls, y_reg, M, acc):
    """Adds the weighted losses (the fp32 bits head_loss_weighted writes, as doubles) and its metric pairs to acc =
    [total, class, regression, sweeps, num0, den0, ...] (float64 device tensor) and counts the sweep; no gradient."""
    ws = _ew_workspace(head.device)
    assert ws.numel() >= _lib.load().lisec_head_loss_weighted_workspace_bytes()
    _lib.check(_lib.load().lisec_head_loss_weighted_eval(ctypes.byref(cfg), ctypes.byref(sw), _lib.ptr(head),
                                                         _lib.ptr(y_cls), _lib.ptr(y_reg), M, _lib.ptr(acc), _lib.ptr(ws),
                                                         ws.numel(), _lib.current_stream()))


def detection_loss_weighted(cfg, sw, head, y_cls, y_reg, M, dhead, loss_out, counts_out, grad_scale=1.0):
    """detection_loss (an _lib.DetectionLossCfg) or detection_iou_loss (an _lib.DetectionIoULossCfg) under the sample
    weights sw; the counts stay unweighted."""
    iou = isinstance(cfg, _lib.DetectionIoULossCfg)
    run = _lib.load().lisec_detection_iou_loss_weighted if iou else _lib.load().lisec_detection_loss_weighted
    ws = _detection_workspace(head.device)
    _lib.check(run(ctypes.byref(cfg), ctypes.byref(sw), _lib.ptr(head), _lib.ptr(y_cls), _lib.ptr(y_reg), M, grad_scale,
                   _lib.ptr(dhead), _lib.ptr(loss_out), _lib.ptr(counts_out), _lib.ptr(ws), ws.numel(),
                   _lib.current_stream()))


def detection_loss_weighted_eval(cfg, sw, head, y_cls, y_reg, M, acc):
    """Adds the [total, class, regression] detection_loss_weighted would write to acc[0:3] and counts the sweep in
    acc[3]; either descriptor, as there."""
    iou = isinstance(cfg, _lib.DetectionIoULossCfg)
    run = _lib.load().lisec_detection_iou_loss_weighted_eval if iou else _lib.load().lisec_detection_loss_weighted_eval
    ws = _detection_workspace(head.device)
    _lib.check(run(ctypes.byref(cfg), ctypes.byref(sw), _lib.ptr(head), _lib.ptr(y_cls), _lib.ptr(y_reg), M,
                   _lib.ptr(acc), _lib.ptr(ws), ws.numel(), _lib.current_stream()))


def detection_metrics(cfg, head, y_cls, y_reg, M, out, accumulate=False):
    """The detection metrics of cfg (an _lib.DetectionMetricsCfg, lisec_detection_metrics_cfg) as pairs of sums over the
    sweep's anchors: out (float64 device tensor) = [num0, den0, num1, den1, ...], stored, or added with accumulate."""
    ws = _ew_workspace(head.device)
    assert ws.numel() >= _lib.load().lisec_detection_metrics_workspace_bytes()
    _lib.check(_lib.load().lisec_detection_metrics(ctypes.byref(cfg), _lib.ptr(head), _lib.ptr(y_cls), _lib.ptr(y_reg), M,
                                                   _lib.ptr(out), 1 if accumulate else 0, _lib.ptr(ws), ws.numel(),
                                                   _lib.current_stream()))


def select_variables(params, names, what):
    """The ParamStore names that `names` selects, in the order given, each once.  names: a string or an iterable of
    ParamStore names and / or the kinds 'kernel', 'bias', 'gamma', 'beta' (each: every variable of that kind, in the
    order of params.specs).  params: a ParamStore, or anything with its `offsets` ({name: ("theta", offset, shape)})
    and, for a kind, its `specs`.  What None means is the caller's business.  KeyError: a name the network does not
    have (a kind of variable that is not trained among them); ValueError: a variable that is not trainable (the
    BatchNormalization moving statistics), "... it cannot be {what}"."""
    chosen = []
    for name in (names,) if isinstance(names, str) else names:
        if name in TRAINABLE_KINDS:
            chosen.extend(n for n, _, kind in params.specs if kind == name)
        elif params.offsets[name][0] != "theta":
            raise ValueError(f"{name} is not a trainable variable: it cannot be {what}")
        else:
            chosen.append(name)
    return list(dict.fromkeys(chosen))


def variable_chunks(params, name):
    """Yields the (offset, count) chunks of one trainable variable: its padded length -- up to the next multiple of 4
    floats; the padding floats of theta are 0, stay 0 and add nothing to a sum -- cut into ceil(n / REG_CHUNK) pieces
    of at most REG_CHUNK floats, ascending.  The chunk rules of include/lisec_hip.h, for every table of this module."""
    _, off, shape = params.offsets[name]
    n = (math.prod(shape) + 3) // 4 * 4
    for start in range(0, n, _lib.REG_CHUNK):
        yield off + start, min(_lib.REG_CHUNK, n - start)


class ChunkTable:
    """Host rows as a device table of `record`s (a ctypes Structure of _lib): `rows`, whose leading fields fill the
    record's in order (the rest of a row is the host's own; the rest of a record stays 0); `offsets`, ascending, the
    place in theta of each row (a row's first field unless given); len(); and `records`, the uint8 device tensor,
    whose data_ptr / numel / numpy the table forwards: it stands where that tensor stood (_lib.ptr, a raw launch)."""

    def __init__(self, record, rows, device, offsets=None):
        self.record, self.rows = record, list(rows)
        self.offsets = [r[0] for r in self.rows] if offsets is None else list(offsets)
        arr = (record * max(len(self.rows), 1))()
        for rec, row in zip(arr, self.rows):
            for (field, _), value in zip(record._fields_, row):
                setattr(rec, field, value)
        self.records = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)

    def __len__(self):
        return len(self.rows)

    def data_ptr(self):
        return self.records.data_ptr()

    def numel(self):
        return self.records.numel()

    def numpy(self):
        return self.records.numpy()

    def span(self, lo, hi):
        """(first, count) of the rows that lie in theta[lo:hi], lo and hi variable boundaries.  The spans of [lo, mid)
        and [mid, hi) are adjacent and together that of [lo, hi): the early update of a step plus the closing one
        visit exactly the rows of one update over everything."""
        first = bisect.bisect_left(self.offsets, lo)
        return first, bisect.bisect_left(self.offsets, hi) - first

    def at(self, first, count, who):
        """The address of record `first`, for a launch over rows [first, first + count); ValueError outside the table."""
        if first < 0 or count < 0 or first + count > len(self):
            raise ValueError(f"{who}: rows [{first}, {first + count}) outside a table of {len(self)}")
        return ctypes.c_void_p(self.records.data_ptr() + first * ctypes.sizeof(self.record))


def reg_chunks(params, coeffs, unwritten=()):
    """The chunk table of lisec_regularize as a host list [(offset, count, l1, l2, flags)], ascending in offset: the
    chunks (variable_chunks) of every variable of coeffs ({ParamStore name: (l1, l2)}) with a pair other than (0, 0).
    unwritten: the names of the variables whose gradient slot no backward pass writes (the gradient is identically 0);
    their chunks carry REG_GRAD_IS_ZERO, so that the term is stored into the slot, not added to what the step before
    left there.  Pure host arithmetic: no device, no library.  KeyError, ValueError: select_variables'."""
    rows, unwritten = [], set(unwritten)
    for name in select_variables(params, coeffs, "regularised"):
        l1, l2 = coeffs[name]
        if l1 == 0 and l2 == 0:
            continue
        flags = _lib.REG_GRAD_IS_ZERO if name in unwritten else 0
        rows.extend((off, count, float(l1), float(l2), flags) for off, count in variable_chunks(params, name))
    rows.sort()
    return rows


def reg_table(chunks, device):
    """reg_chunks' list as the device table of lisec_regularize (a ChunkTable of lisec_reg_chunk records); a row may
    leave the flags out (0)."""
    return ChunkTable(_lib.RegChunk, chunks, device)


def reg_workspace(n_chunks, device):
    return torch.empty(_lib.load().lisec_regularize_workspace_bytes(int(n_chunks)), dtype=torch.uint8, device=device)


def regularize(theta, grad, table, n_chunks, penalty, workspace, first=0, accumulate=False, loss_total=None):
    """lisec_regularize over chunks [first, first + n_chunks) of `table` (reg_table; offsets relative to theta / grad as
    given): grad += 2*l2*w + l1*sign(w) (grad None: the penalty alone), penalty (float64[1] device tensor) = P, or += P
    with accumulate, and loss_total[0] (float32 device tensor, or None) = float32(loss_total[0] + penalty)."""
    chunks = table.at(first, int(n_chunks), "regularize")
    _lib.check(_lib.load().lisec_regularize(_lib.ptr(theta), _lib.ptr(grad), chunks, int(n_chunks), _lib.ptr(penalty),
                                            1 if accumulate else 0, _lib.ptr(loss_total), _lib.ptr(workspace),
                                            workspace.numel(), _lib.current_stream()))


def sgd_nesterov_step(theta, grad, velocity, lr_t, momentum):
    _lib.check(_lib.load().lisec_sgd_nesterov_step(_lib.ptr(theta), _lib.ptr(grad), _lib.ptr(velocity),
                                                   theta.numel(), lr_t, momentum, _lib.current_stream()))


def sgd_nesterov_step_dev(theta, grad, velocity, lr, decay, momentum, state, advance=True):
    """state: int64[2] device tensor {iterations, 0}; lr_t is derived on the device (graph-replayable).
    advance=False: a part of the variables ahead of the rest of the step (the iteration count is left alone)."""
    fn = _lib.load().lisec_sgd_nesterov_step_dev if advance else _lib.load().lisec_sgd_nesterov_step_dev_part
    _lib.check(fn(_lib.ptr(theta), _lib.ptr(grad), _lib.ptr(velocity), theta.numel(), float(lr), float(decay), momentum,
                  _lib.ptr(state), _lib.current_stream()))


def sgd_step_dev(theta, grad, velocity, lr, decay, momentum, nesterov, state, advance=True):
    """tf.keras SGD on the device iteration count (lisec_sgd_step_dev): velocity is None exactly when momentum == 0."""
    _lib.check(_lib.load().lisec_sgd_step_dev(_lib.ptr(theta), _lib.ptr(grad), _lib.ptr(velocity), theta.numel(),
                                              float(lr), float(decay), float(momentum), 1 if nesterov else 0,
                                              _lib.ptr(state), 1 if advance else 0, _lib.current_stream()))


def adam_step_dev(theta, grad, m, v, vhat, lr, decay, beta_1, beta_2, epsilon, state, advance=True):
    """tf.keras Adam on the device iteration count (lisec_adam_step_dev); vhat not None: AMSGrad."""
    _lib.check(_lib.load().lisec_adam_step_dev(_lib.ptr(theta), _lib.ptr(grad), _lib.ptr(m), _lib.ptr(v), _lib.ptr(vhat),
                                               theta.numel(), float(lr), float(decay), float(beta_1), float(beta_2),
                                               float(epsilon), _lib.ptr(state), 1 if advance else 0, _lib.current_stream()))


def lr_schedule_set(dev_desc, desc):
    """Stream-ordered write of the learning-rate descriptor `desc` (an _lib.LrSchedule, validated by the library) into
    dev_desc, a device buffer of ctypes.sizeof(_lib.LrSchedule) bytes (lisec_lr_schedule_set)."""
    _lib.check(_lib.load().lisec_lr_schedule_set(_lib.ptr(dev_desc), ctypes.byref(desc), _lib.current_stream()))


def lr_schedule_eval(dev_desc, state, n, out):
    """out[k] = lr_t at iteration state[0] + k, k < n (lisec_lr_schedule_eval; state is not advanced)."""
    _lib.check(_lib.load().lisec_lr_schedule_eval(_lib.ptr(dev_desc), _lib.ptr(state), int(n), _lib.ptr(out),
                                                  _lib.current_stream()))


def sgd_step_sched(theta, grad, velocity, dev_desc, momentum, nesterov, state, advance=True):
    """sgd_step_dev with lr_t from the device descriptor dev_desc (lisec_sgd_step_sched)."""
    _lib.check(_lib.load().lisec_sgd_step_sched(_lib.ptr(theta), _lib.ptr(grad), _lib.ptr(velocity), theta.numel(),
                                                _lib.ptr(dev_desc), float(momentum), 1 if nesterov else 0,
                                                _lib.ptr(state), 1 if advance else 0, _lib.current_stream()))


def adam_step_sched(theta, grad, m, v, vhat, dev_desc, beta_1, beta_2, epsilon, state, advance=True):
    """adam_step_dev with lr_t from the device descriptor dev_desc (lisec_adam_step_sched); vhat not None: AMSGrad."""
    _lib.check(_lib.load().lisec_adam_step_sched(_lib.ptr(theta), _lib.ptr(grad), _lib.ptr(m), _lib.ptr(v),
                                                 _lib.ptr(vhat), theta.numel(), _lib.ptr(dev_desc), float(beta_1),
                                                 float(beta_2), float(epsilon), _lib.ptr(state), 1 if advance else 0,
                                                 _lib.current_stream()))


# ---- the other tf.keras optimizers (csrc/optim_keras.hip): *_dev take (lr, decay), *_sched the device descriptor -------
def rmsprop_step_dev(theta, grad, rms, mom, mg, lr, decay, rho, momentum, epsilon, state, advance=True):
    """tf.keras RMSprop (lisec_rmsprop_step_dev): mom is None exactly when momentum == 0, mg exactly when not centered."""
    P = _lib.ptr
    _lib.check(_lib.load().lisec_rmsprop_step_dev(P(theta), P(grad), P(rms), P(mom), P(mg), theta.numel(), float(lr),
                                                  float(decay), float(rho), float(momentum), float(epsilon),
                                                  0 if mg is None else 1, P(state), 1 if advance else 0,
                                                  _lib.current_stream()))


def rmsprop_step_sched(theta, grad, rms, mom, mg, dev_desc, rho, momentum, epsilon, state, advance=True):
    P = _lib.ptr
    _lib.check(_lib.load().lisec_rmsprop_step_sched(P(theta), P(grad), P(rms), P(mom), P(mg), theta.numel(), P(dev_desc),
                                                    float(rho), float(momentum), float(epsilon), 0 if mg is None else 1,
                                                    P(state), 1 if advance else 0, _lib.current_stream()))


def adagrad_step_dev(theta, grad, accumulator, lr, decay, epsilon, state, advance=True):
    P = _lib.ptr
    _lib.check(_lib.load().lisec_adagrad_step_dev(P(theta), P(grad), P(accumulator), theta.numel(), float(lr),
                                                  float(decay), float(epsilon), P(state), 1 if advance else 0,
                                                  _lib.current_stream()))


def adagrad_step_sched(theta, grad, accumulator, dev_desc, epsilon, state, advance=True):
    P = _lib.ptr
    _lib.check(_lib.load().lisec_adagrad_step_sched(P(theta), P(grad), P(accumulator), theta.numel(), P(dev_desc),
                                                    float(epsilon), P(state), 1 if advance else 0, _lib.current_stream()))


def adadelta_step_dev(theta, grad, accum_grad, accum_var, lr, decay, rho, epsilon, state, advance=True):
    P = _lib.ptr
    _lib.check(_lib.load().lisec_adadelta_step_dev(P(theta), P(grad), P(accum_grad), P(accum_var), theta.numel(),
                                                   float(lr), float(decay), float(rho), float(epsilon), P(state),
                                                   1 if advance else 0, _lib.current_stream()))


def adadelta_step_sched(theta, grad, accum_grad, accum_var, dev_desc, rho, epsilon, state, advance=True):
    P = _lib.ptr
    _lib.check(_lib.load().lisec_adadelta_step_sched(P(theta), P(grad), P(accum_grad), P(accum_var), theta.numel(),
                                                     P(dev_desc), float(rho), float(epsilon), P(state),
                                                     1 if advance else 0, _lib.current_stream()))


def adamax_step_dev(theta, grad, m, v, lr, decay, beta_1, beta_2, epsilon, state, advance=True):
    P = _lib.ptr
    _lib.check(_lib.load().lisec_adamax_step_dev(P(theta), P(grad), P(m), P(v), theta.numel(), float(lr), float(decay),
                                                 float(beta_1), float(beta_2), float(epsilon), P(state),
                                                 1 if advance else 0, _lib.current_stream()))


def adamax_step_sched(theta, grad, m, v, dev_desc, beta_1, beta_2, epsilon, state, advance=True):
    P = _lib.ptr
    _lib.check(_lib.load().lisec_adamax_step_sched(P(theta), P(grad), P(m), P(v), theta.numel(), P(dev_desc),
                                                   float(beta_1), float(beta_2), float(epsilon), P(state),
                                                   1 if advance else 0, _lib.current_stream()))


def nadam_step_dev(theta, grad, m, v, momentum_cache, lr, beta_1, beta_2, epsilon, schedule_decay, state, advance=True):
    """tf.keras Nadam (lisec_nadam_step_dev): momentum_cache is a float32 device scalar, advanced with the iteration
    count; lr is not decayed."""
    P = _lib.ptr
    _lib.check(_lib.load().lisec_nadam_step_dev(P(theta), P(grad), P(m), P(v), P(momentum_cache), theta.numel(),
                                                float(lr), float(beta_1), float(beta_2), float(epsilon),
                                                float(schedule_decay), P(state), 1 if advance else 0,
                                                _lib.current_stream()))


def nadam_step_sched(theta, grad, m, v, momentum_cache, dev_desc, beta_1, beta_2, epsilon, schedule_decay, state,
                     advance=True):
    P = _lib.ptr
    _lib.check(_lib.load().lisec_nadam_step_sched(P(theta), P(grad), P(m), P(v), P(momentum_cache), theta.numel(),
                                                  P(dev_desc), float(beta_1), float(beta_2), float(epsilon),
                                                  float(schedule_decay), P(state), 1 if advance else 0,
                                                  _lib.current_stream()))


def fold_depth(x, out, D, HW, C, inverse=False, mask=None):
    """(D,H,W,C) <-> (H,W,C*D) (Permute + Reshape of model_training.py:242-243); inverse: gradient, ReLU-gated by mask."""
    _lib.check(_lib.load().lisec_fold_depth(_lib.ptr(x), _lib.ptr(out), D, HW, C, 1 if inverse else 0, _lib.ptr(mask),
                                            _lib.current_stream()))
    return out


def scale_(x, s):
    _lib.check(_lib.load().lisec_scale(_lib.ptr(x), x.numel(), s, _lib.current_stream()))


def grad_accumulate(grad, acc, mode, scale=None):
    """lisec_grad_accumulate over the whole of `grad` and `acc` (float32 device tensors of one length, a multiple of 4;
    slices of the flat gradient buffer and of the accumulator at the same offset): mode _lib.ACC_BEGIN acc = grad,
    ACC_ADD acc = acc + grad, ACC_END grad = (acc + grad) * scale[0] with scale a float32 device tensor the kernel
    reads.  fp32 adds in call order, then one fp32 multiply, never contracted (include/lisec_hip.h)."""
    if grad.numel() != acc.numel():
        raise ValueError(f"grad_accumulate: {grad.numel()} gradient floats, {acc.numel()} accumulator floats")
    _lib.check(_lib.load().lisec_grad_accumulate(_lib.ptr(grad), _lib.ptr(acc), grad.numel(), int(mode), _lib.ptr(scale),
                                                 _lib.current_stream()))


def weight_average(theta, avg, desc, state, state_bias=0):
    """One averaging pass of lisec_weight_average over the whole of `theta` (read) and `avg` (float32 device tensors of
    one length, a multiple of 4): desc an _lib.WeightAverage (host; copied into the launch), state the device iteration
    count, read as state[0] + state_bias -- 0 in front of the update that advances it, -1 behind it.  EMA: a <- a -
    (a - w)*c, SWA: a <- (a*m + w)/(m + 1) on a snapshot step, every op rounded to fp32 on its own (include/lisec_hip.h)."""
    if theta.numel() != avg.numel():
        raise ValueError(f"weight_average: {theta.numel()} variables, {avg.numel()} averages")
    _lib.check(_lib.load().lisec_weight_average(_lib.ptr(theta), _lib.ptr(avg), theta.numel(), ctypes.byref(desc),
                                                _lib.ptr(state), int(state_bias), _lib.current_stream()))


def weight_swap(a, b):
    """a <-> b by content, bit for bit (lisec_weight_swap; float32 device tensors of one length, a multiple of 4)."""
    if a.numel() != b.numel():
        raise ValueError(f"weight_swap: {a.numel()} and {b.numel()} floats")
    _lib.check(_lib.load().lisec_weight_swap(_lib.ptr(a), _lib.ptr(b), a.numel(), _lib.current_stream()))


def weight_average_eval(desc, state, k, c_out=None, m_out=None):
    """For j < k, at iteration state[0] + j: EMA c_out[j] = c (float32), SWA m_out[j] = m or -1 off a snapshot (int64)
    (lisec_weight_average_eval; state is not advanced)."""
    _lib.check(_lib.load().lisec_weight_average_eval(ctypes.byref(desc), _lib.ptr(state), int(k), _lib.ptr(c_out),
                                                     _lib.ptr(m_out), _lib.current_stream()))


def decay_chunks(params, names=None):
    """The chunk table of lisec_weight_decay as a host list [(offset, count)], ascending in offset: the chunks
    (variable_chunks) of every variable that `names` selects (select_variables); None -- every trainable variable.
    params: a ParamStore, or anything with its `specs` and `offsets`.  Pure host arithmetic: no device, no library."""
    chosen = select_variables(params, TRAINABLE_KINDS if names is None else names, "decayed")
    return sorted(chunk for name in chosen for chunk in variable_chunks(params, name))


def decay_table(chunks, device):
    """decay_chunks' list as the device table of lisec_weight_decay (a ChunkTable of lisec_decay_chunk records)."""
    return ChunkTable(_lib.DecayChunk, chunks, device)


def weight_decay(theta, table, n_chunks, coeff, state, first=0):
    """lisec_weight_decay over chunks [first, first + n_chunks) of `table` (decay_table; offsets relative to theta as
    given): w <- w - wd_t*w, a float32 multiply and a float32 subtraction, wd_t = float32(schedule(state[0])) of the
    device descriptor `coeff` (lr_schedule_set; its decay 0).  state is read, never advanced."""
    chunks = table.at(first, int(n_chunks), "weight_decay")
    _lib.check(_lib.load().lisec_weight_decay(_lib.ptr(theta), chunks, int(n_chunks), _lib.ptr(coeff), _lib.ptr(state),
                                              _lib.current_stream()))


def weight_decay_eval(coeff, state, k, out):
    """out[j] = wd_t at iteration state[0] + j, j < k (lisec_weight_decay_eval; state is not advanced)."""
    _lib.check(_lib.load().lisec_weight_decay_eval(_lib.ptr(coeff), _lib.ptr(state), int(k), _lib.ptr(out),
                                                   _lib.current_stream()))


LAMB_BLOCKS = _lib.LAMB_BLOCKS                 # the widest grid of a LAMB pass: past it the workgroups stride over the table


def lamb_chunks(params, exclude_from_weight_decay=None, exclude_from_layer_adaptation=None):
    """The tables of lisec_lamb_step_* as host lists, both ascending in offset: (chunk rows [(offset, count, var,
    flags)], variable rows [(first_chunk, n_chunks, offset, name)]).  EVERY trainable variable is in them, cut by
    variable_chunks (the padding floats have a zero gradient and add nothing to either norm); var is the index of the
    chunk's row in the variable rows; flags has LAMB_DECAYED unless exclude_from_weight_decay selects the variable and
    LAMB_ADAPTED unless exclude_from_layer_adaptation does -- None there: the list of exclude_from_weight_decay, as in
    tfa; None for both: no variable.  Both lists take what select_variables takes.  Pure host arithmetic."""
    if exclude_from_layer_adaptation is None:
        exclude_from_layer_adaptation = exclude_from_weight_decay
    undecayed, unadapted = (set(select_variables(params, () if names is None else names, "excluded from an update"))
                            for names in (exclude_from_weight_decay, exclude_from_layer_adaptation))
    chunks, variables = [], []
    for name in sorted(select_variables(params, TRAINABLE_KINDS, "updated"), key=lambda n: params.offsets[n][1]):
        flags = (0 if name in undecayed else _lib.LAMB_DECAYED) | (0 if name in unadapted else _lib.LAMB_ADAPTED)
        first = len(chunks)
        chunks.extend((off, count, len(variables), flags) for off, count in variable_chunks(params, name))
        variables.append((first, len(chunks) - first, params.offsets[name][1], name))
    return chunks, variables


class LambTable:
    """lamb_chunks' lists on the device: `chunks` (a ChunkTable of lisec_lamb_chunk records), `variables` (one of
    lisec_lamb_var records, keyed by the offset of each variable's first chunk), their lengths n_chunks / n_vars and
    `names`, the variables' (empty when the rows carry none)."""

    def __init__(self, chunks, variables, device):
        self.chunks = ChunkTable(_lib.LambChunk, chunks, device)
        self.variables = ChunkTable(_lib.LambVar, variables, device, offsets=[chunks[v[0]][0] for v in variables])
        self.n_chunks, self.n_vars = len(chunks), len(variables)
        self.names = [v[3] for v in variables if len(v) > 3]


def lamb_table(chunks, variables, device):
    """lamb_chunks' two lists as the device tables of lisec_lamb_step_* (a LambTable); a variable row may be just
    (first_chunk, n_chunks)."""
    return LambTable(chunks, variables, device)


def lamb_workspace(n_chunks, n_vars, device):
    """The workspace of lisec_lamb_step_* for a table of n_chunks chunks and n_vars variables (uint8 tensor)."""
    return torch.empty(_lib.load().lisec_lamb_workspace_bytes(int(n_chunks), int(n_vars)), dtype=torch.uint8,
                       device=device)


def _lamb_range(table, ratios, first, n_chunks, first_var, n_vars):
    """The rows of a launch as ints, None: to the end; ValueError outside either table or past the ratios."""
    n_chunks = table.n_chunks - first if n_chunks is None else int(n_chunks)
    n_vars = table.n_vars - first_var if n_vars is None else int(n_vars)
    table.chunks.at(first, n_chunks, "lamb chunks")
    table.variables.at(first_var, n_vars, "lamb variables")
    if first_var + n_vars > ratios.numel():
        raise ValueError(f"lamb: variables [{first_var}, {first_var + n_vars}) with {ratios.numel()} ratios")
    return int(first), n_chunks, int(first_var), n_vars


def lamb_step_dev(theta, grad, m, v, lr, decay, weight_decay_rate, beta_1, beta_2, epsilon, state, advance=True, *,
                  table, ratios, workspace, first=0, n_chunks=None, first_var=0, n_vars=None):
    """LAMB on the device iteration count (lisec_lamb_step_dev) over chunks [first, first + n_chunks) and variables
    [first_var, first_var + n_vars) of `table` (lamb_table; None: to the end; the chunks must be those of the
    variables).  theta, grad, m, v are the WHOLE buffers the table's offsets count from; ratios (float32 device tensor,
    one per variable of the table) receives r of the variables of the range; workspace: lamb_workspace."""
    first, n_chunks, first_var, n_vars = _lamb_range(table, ratios, first, n_chunks, first_var, n_vars)
    P = _lib.ptr
    _lib.check(_lib.load().lisec_lamb_step_dev(P(theta), P(grad), P(m), P(v), P(table.chunks), first, n_chunks,
                                               P(table.variables), first_var, n_vars, P(ratios), P(workspace),
                                               workspace.numel(), float(lr), float(decay), float(weight_decay_rate),
                                               float(beta_1), float(beta_2), float(epsilon), P(state),
                                               1 if advance else 0, _lib.current_stream()))


def lamb_step_sched(theta, grad, m, v, dev_desc, weight_decay_rate, beta_1, beta_2, epsilon, state, advance=True, *,
                    table, ratios, workspace, first=0, n_chunks=None, first_var=0, n_vars=None):
    """lamb_step_dev with lr_t from the device descriptor dev_desc (lisec_lamb_step_sched)."""
    first, n_chunks, first_var, n_vars = _lamb_range(table, ratios, first, n_chunks, first_var, n_vars)
    P = _lib.ptr
    _lib.check(_lib.load().lisec_lamb_step_sched(P(theta), P(grad), P(m), P(v), P(table.chunks), first, n_chunks,
                                                 P(table.variables), first_var, n_vars, P(ratios), P(workspace),
                                                 workspace.numel(), P(dev_desc), float(weight_decay_rate),
                                                 float(beta_1), float(beta_2), float(epsilon), P(state),
                                                 1 if advance else 0, _lib.current_stream()))


def clip_chunks(params):
    """The tables of lisec_grad_clip_* as host lists: lamb_chunks without exclusions -- every trainable variable, cut by
    variable_chunks, each chunk with its variable's index (the flags are ignored by the clipping passes).  They become
    device tables through lamb_table.  Pure host arithmetic."""
    return lamb_chunks(params)


def clip_workspace(n_chunks, device):
    """The workspace of lisec_grad_clip_norm / _global_norm_* for a table of n_chunks chunks (uint8 tensor)."""
    return torch.empty(_lib.load().lisec_grad_clip_workspace_bytes(int(n_chunks)), dtype=torch.uint8, device=device)


def _clip_chunk_range(table, first, n_chunks):
    n_chunks = table.n_chunks - first if n_chunks is None else int(n_chunks)
    table.chunks.at(first, n_chunks, "grad_clip chunks")
    return int(first), n_chunks


def grad_clip_value(grad, clip, *, table, first=0, n_chunks=None):
    """g <- min(max(g, -clip), clip) where g is ordered, a NaN keeps its bits (lisec_grad_clip_value) over chunks [first,
    first + n_chunks) of `table` (lamb_table of clip_chunks; None: to the end).  grad is the WHOLE buffer the table's
    offsets count from."""
    first, n_chunks = _clip_chunk_range(table, first, n_chunks)
    _lib.check(_lib.load().lisec_grad_clip_value(_lib.ptr(grad), _lib.ptr(table.chunks), first, n_chunks, float(clip),
                                                 _lib.current_stream()))


def grad_clip_norm(grad, clip, *, table, scales, norms, workspace, first=0, n_chunks=None, first_var=0, n_vars=None):
    """Every variable of the range scaled so that its L2 norm is at most clip (lisec_grad_clip_norm) over chunks [first,
    first + n_chunks) and variables [first_var, first_var + n_vars) of `table` (None: to the end; the chunks must be
    those of the variables).  scales / norms (float32 device tensors, one per variable of the table) receive each
    variable's scale and norm; workspace: clip_workspace."""
    first, n_chunks, first_var, n_vars = _lamb_range(table, scales, first, n_chunks, first_var, n_vars)
    if first_var + n_vars > norms.numel():
        raise ValueError(f"grad_clip_norm: variables [{first_var}, {first_var + n_vars}) with {norms.numel()} norms")
    P = _lib.ptr
    _lib.check(_lib.load().lisec_grad_clip_norm(P(grad), P(table.chunks), first, n_chunks, P(table.variables), first_var,
                                                n_vars, float(clip), P(scales), P(norms), P(workspace), workspace.numel(),
                                                _lib.current_stream()))


def grad_clip_global_norm_partials(grad, *, table, workspace, first=0, n_chunks=None):
    """The per-chunk sums of squares of chunks [first, first + n_chunks) into their slots of the workspace
    (lisec_grad_clip_global_norm_partials): a part of the global norm, ahead of grad_clip_global_norm_finish."""
    first, n_chunks = _clip_chunk_range(table, first, n_chunks)
    _lib.check(_lib.load().lisec_grad_clip_global_norm_partials(_lib.ptr(grad), _lib.ptr(table.chunks), first, n_chunks,
                                                                _lib.ptr(workspace), workspace.numel(),
                                                                _lib.current_stream()))


def grad_clip_global_norm_finish(grad, clip, *, table, scales, norms, workspace, first=0, n_chunks=None):
    """Adds the partials of ALL chunks of `table`, stores scales[0] / norms[0] and scales chunks [first, first + n_chunks)
    (None: to the end) by scales[0] (lisec_grad_clip_global_norm_finish)."""
    first, n_chunks = _clip_chunk_range(table, first, n_chunks)
    P = _lib.ptr
    _lib.check(_lib.load().lisec_grad_clip_global_norm_finish(P(grad), P(table.chunks), table.n_chunks, first, n_chunks,
                                                              float(clip), P(scales), P(norms), P(workspace),
                                                              workspace.numel(), _lib.current_stream()))


def grad_clip_global_norm(grad, clip, *, table, scales, norms, workspace):
    """The whole gradient scaled so that its L2 norm over every variable of `table` is at most clip: the partials of
    every chunk, then grad_clip_global_norm_finish over every chunk."""
    grad_clip_global_norm_partials(grad, table=table, workspace=workspace)
    grad_clip_global_norm_finish(grad, clip, table=table, scales=scales, norms=norms, workspace=workspace)


BN_STATISTICS = {"mean": _lib.BN_STATS_MEAN, "pooled": _lib.BN_STATS_POOLED}     # the rules of bn_recalibrate_finish
VFE_BN_LAYERS = ("vfe1.bn", "vfe2.bn", "fcn.bn")      # finalised by the VFE kernel; every other layer by a conv sink


def bn_statistics(statistics):
    """LISEC_BN_STATS_* of 'mean' / 'pooled'; ValueError for anything else.  No device, no library."""
    try:
        return BN_STATISTICS[statistics]
    except (KeyError, TypeError):
        raise ValueError(f"statistics must be 'mean' or 'pooled', not {statistics!r}") from None


def bn_recal_rows(params):
    """The table of lisec_bn_recalibrate_* as a host list [(mean_off, var_off, C, family)], one row per
    BatchNormalization layer in forward order: the offsets of its moving statistics in ParamStore.state and the family
    of the finaliser that updates them in a training forward (_lib.BN_FINALIZER_VFE for the three VFE layers,
    BN_FINALIZER_CONV for the rest).  params: a ParamStore, or anything with its `specs` and `offsets`.  Pure host
    arithmetic."""
    rows = []
    for name, shape, kind in params.specs:
        if kind != "moving_mean":
            continue
        prefix = name[:-len(".moving_mean")]
        family = _lib.BN_FINALIZER_VFE if prefix in VFE_BN_LAYERS else _lib.BN_FINALIZER_CONV
        rows.append((params.offsets[name][1], params.offsets[prefix + ".moving_variance"][1], int(shape[0]), family))
    return rows


class BnRecalTable:
    """rows [(mean_off, var_off, C, coef)] as the HOST table of lisec_bn_recalibrate_* (the library validates it and
    copies it into each launch); `channels` = the sum of C: acc holds 3 * channels doubles."""

    def __init__(self, rows):
        self.n_entries = len(rows)
        self.channels = sum(int(r[2]) for r in rows)
        self.records = (_lib.BnRecalEntry * max(len(rows), 1))()
        for rec, (mean_off, var_off, C, coef) in zip(self.records, rows):
            rec.mean_off, rec.var_off, rec.C, rec.coef = int(mean_off), int(var_off), int(C), float(coef)


def bn_recal_table(rows):
    """bn_recal_rows' list as a BnRecalTable, each family replaced by its coefficient 1 - momentum as that finaliser
    computes it (lisec_bn_recalibrate_coef: the constants live next to the kernels)."""
    lib = _lib.load()
    return BnRecalTable([(m, v, C, lib.lisec_bn_recalibrate_coef(int(family))) for m, v, C, family in rows])


def bn_recal_acc(table, device):
    """The zeroed accumulator of a recalibration: float64[3 * channels], the planes S1, S2, Sq (include/lisec_hip.h)."""
    return torch.zeros(3 * table.channels, dtype=torch.float64, device=device)


def _bn_recal_check(state, table, acc):
    if state.dtype != torch.float32 or acc.dtype != torch.float64:
        raise ValueError("bn_recalibrate: state must be float32 and acc float64")
    if acc.numel() < 3 * table.channels:
        raise ValueError(f"bn_recalibrate: acc holds {acc.numel()} doubles, the table needs {3 * table.channels}")
    for rec in table.records[:table.n_entries]:
        if max(rec.mean_off, rec.var_off) + rec.C > state.numel():
            raise ValueError(f"bn_recalibrate: a record of {rec.C} channels at ({rec.mean_off}, {rec.var_off}) lies "
                             f"outside a state of {state.numel()} floats")


def bn_recalibrate_take(state, table, acc):
    """One sweep of a recalibration (lisec_bn_recalibrate_take), behind its forward(training=True) over a zeroed
    `state`: per channel S1 += m, S2 += v, Sq += m*m in fp64 with m, v = state / coef, and the two floats of state are
    zeroed for the next sweep.  table: a BnRecalTable; acc: bn_recal_acc."""
    _bn_recal_check(state, table, acc)
    _lib.check(_lib.load().lisec_bn_recalibrate_take(_lib.ptr(state), table.records, table.n_entries, _lib.ptr(acc),
                                                     _lib.current_stream()))


def bn_recalibrate_finish(state, table, acc, sweeps, statistics="mean"):
    """The moving statistics of `sweeps` takes (lisec_bn_recalibrate_finish): mean = S1/k; 'mean': var = S2/k,
    'pooled': var = max(0, S2/k + Sq/k - mean*mean); each rounded once to float32 into state.  acc is only read."""
    rule = bn_statistics(statistics)
    _bn_recal_check(state, table, acc)
    _lib.check(_lib.load().lisec_bn_recalibrate_finish(_lib.ptr(state), table.records, table.n_entries, _lib.ptr(acc),
                                                       int(sweeps), rule, _lib.current_stream()))


def conv_field_forward_workspace_bytes(g, row_capacity):
    return _lib.load().lisec_conv_field_forward_workspace_bytes(ctypes.byref(g), row_capacity)


def conv_field_forward(g, vout, delta, sample, wp, out, workspace, bias=None, sink=None):
    """First Conv3D over the VFE's compact output (constant + voxel rows) instead of the dense grid; sample: the
    VoxelSample the VFE ran on; workspace: uint8 tensor of conv_field_forward_workspace_bytes(g, sample.cap)."""
    _lib.check(_lib.load().lisec_conv_field_forward(
        ctypes.byref(g), _lib.ptr(vout), _lib.ptr(delta), _lib.ptr(sample.info), _lib.ptr(sample.coords),
        _lib.ptr(sample.cell_voxel), sample.cap, _lib.ptr(wp), _lib.ptr(bias), _lib.ptr(out),
        sink.ref if sink is not None else None, _lib.ptr(workspace), workspace.numel(), _lib.current_stream()))
    return out


def tap_sums(g, dy, S, workspace):
    _lib.check(_lib.load().lisec_conv_tap_sums(ctypes.byref(g), _lib.ptr(dy), _lib.ptr(S), _lib.ptr(workspace),
                                               workspace.numel() * workspace.element_size(), _lib.current_stream()))


def tap_sums_bn(g, dz, y, bnstate, coef, dy, S, workspace):
    """tap_sums fused with bn_backward_apply_coef(relu=False) in front of it: dy (may be dz) is written, S summed."""
    _lib.check(_lib.load().lisec_conv_tap_sums_bn(ctypes.byref(g), _lib.ptr(dz), _lib.ptr(y), _lib.ptr(bnstate),
                                                  _lib.ptr(coef), _lib.ptr(dy), _lib.ptr(S), _lib.ptr(workspace),
                                                  workspace.numel() * workspace.element_size(), _lib.current_stream()))


def tap_sums_finish(g, workspace, S):
    """Second half of tap_sums_bn(..., S=None): the per-line sums left in `workspace` summed into S."""
    _lib.check(_lib.load().lisec_conv_tap_sums_finish(ctypes.byref(g), _lib.ptr(workspace),
                                                      workspace.numel() * workspace.element_size(), _lib.ptr(S),
                                                      _lib.current_stream()))


def tap_sums_workspace_bytes(g):
    return _lib.load().lisec_conv_tap_sums_workspace_bytes(ctypes.byref(g))


def const_field_grads(W, S, cvec, ntaps, cin, cout, dW=None, g_all=None, cvec_row=None, cvec_row_max=0):
    _lib.check(_lib.load().lisec_const_field_grads(_lib.ptr(W), _lib.ptr(S), _lib.ptr(cvec), _lib.ptr(cvec_row),
                                                   cvec_row_max, ntaps, cin, cout, _lib.ptr(dW), _lib.ptr(g_all),
                                                   _lib.current_stream()))


def head_compose(up_kernel, up_bias, head_w, taps, cin, cup, Wc, tap_stride, c_stride, bias_in=None, bias_out=None):
    """Composite kernel of one upsampling branch and the heads (lisec_head_compose): Wc[tap*tap_stride + c*c_stride + j]."""
    _lib.check(_lib.load().lisec_head_compose(_lib.ptr(up_kernel), _lib.ptr(up_bias), _lib.ptr(head_w), taps, cin, cup,
                                              tap_stride, c_stride, _lib.ptr(Wc), _lib.ptr(bias_in), _lib.ptr(bias_out),
                                              _lib.current_stream()))


def head_compose_backward(G, tap_stride, c_stride, up_kernel, up_bias, head_w, S, taps, cin, cup, d_up_kernel, d_up_bias,
                          d_head_w):
    _lib.check(_lib.load().lisec_head_compose_backward(_lib.ptr(G), tap_stride, c_stride, _lib.ptr(up_kernel),
                                                       _lib.ptr(up_bias), _lib.ptr(head_w), _lib.ptr(S), taps, cin, cup,
                                                       _lib.ptr(d_up_kernel),
                                                       _lib.ptr(d_up_bias), _lib.ptr(d_head_w), _lib.current_stream()))


class HeadShuffle:
    """lisec_head_shuffle over fixed branch buffers: head += pixel-shuffled T_b (forward) / T_b = shuffled dhead (backward)."""

    def __init__(self, Ho, Wo, branches):
        self.Ho, self.Wo, self.n = Ho, Wo, len(branches)
        self.keep = [t for t, _ in branches]
        self.T = (ctypes.c_void_p * self.n)(*[t.data_ptr() for t, _ in branches])
        self.ps = (ctypes.c_int * self.n)(*[p for _, p in branches])

    def run(self, head, backward=False):
        _lib.check(_lib.load().lisec_head_shuffle(_lib.ptr(head), self.Ho, self.Wo, self.n, self.T, self.ps,
                                                  1 if backward else 0, _lib.current_stream()))


# ---- many-box detection output (include/lisec_hip.h section 5b) -----------------------------------------------------------
def detect_params(score_threshold=-math.inf, sigmoid_scores=False, pre_nms_top_n=1000, max_boxes=100, iou_threshold=0.1,
                  iou_mode=1, inside_only=True):
    """lisec_detect_cfg; iou_mode 0 = LISEC_IOU_3D, 1 = LISEC_IOU_BEV.  Nothing is checked here: lisec_detect refuses."""
    d = _lib.DetectCfg()
    d.score_threshold, d.iou_threshold = float(score_threshold), float(iou_threshold)
    d.sigmoid_scores, d.inside_only, d.iou_mode = int(bool(sigmoid_scores)), int(bool(inside_only)), int(iou_mode)
    d.pre_nms_top_n, d.max_boxes = int(pre_nms_top_n), int(max_boxes)
    return d


def detect(cfg, det, cls, reg):
    """lisec_detect on device maps cls (outX, outY, >= 2) and reg (outX, outY, >= 14) float32 with unit element stride.
    Returns device tensors (boxes (max_boxes, 7) float64, scores (max_boxes,) float64, index (max_boxes,) int32, count (2,)
    int32 = kept, passing), zero past the kept rows, without waiting for the GPU."""
    lib, dev = _lib.load(), cls.device
    nbytes = lib.lisec_detect_workspace_bytes(ctypes.byref(cfg), ctypes.byref(det))
    if nbytes == 0:
        raise _lib.LisecError(f"lisec C ABI error -1: {lib.lisec_last_error().decode()}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    boxes = torch.zeros((det.max_boxes, 7), dtype=torch.float64, device=dev)
    scores = torch.zeros(det.max_boxes, dtype=torch.float64, device=dev)
    index = torch.zeros(det.max_boxes, dtype=torch.int32, device=dev)
    count = torch.zeros(2, dtype=torch.int32, device=dev)
    _lib.check(lib.lisec_detect(ctypes.byref(cfg), ctypes.byref(det), _lib.ptr(cls), cls.stride(1), _lib.ptr(reg),
                                reg.stride(1), _lib.ptr(ws), nbytes, _lib.ptr(boxes), _lib.ptr(scores), _lib.ptr(index),
                                _lib.ptr(count), _lib.current_stream()))
    return boxes, scores, index, count


# ---- training-time augmentation (include/lisec_hip.h section 5c) ----------------------------------------------------------
def augment_params(rot_box=math.pi / 10, sigma=(1.0, 1.0, 0.0), scale=(0.95, 1.05), rot_global=math.pi / 4, attempts=10):
    """lisec_augment_params with VoxelNet's defaults (section 3.3 of the paper; z noise 0: the grid is 2 m tall)."""
    p = _lib.AugmentParams()
    p.rot_box, p.rot_global, p.attempts = float(rot_box), float(rot_global), int(attempts)
    p.scale_lo, p.scale_hi = float(scale[0]), float(scale[1])
    for i in range(3):
        p.sigma[i] = float(sigma[i])
    return p


def _int32_count(n_boxes):
    if n_boxes.dtype != torch.int32 or n_boxes.numel() != 1 or not n_boxes.is_cuda:
        raise ValueError("a device-side box count is one int32 on the device")
    return _lib.ptr(n_boxes)


def augment_draw(boxes, params, seed=0, item=0, epoch=0, n_boxes=None):
    """lisec_augment_draw on device rows boxes (B, 7) float64.  Returns device tensors (transforms (B, 4), global (2,),
    boxes_out (B, 7), attempt (B,) int32, draws (4 + 8 B,) uint32 held as int32 bits).  n_boxes: a device int32 (1,) holding
    the number of rows that count (lisec_augment_draw_n; B bounds it): the outputs are zero past it."""
    B, dev = int(boxes.shape[0]), boxes.device
    new = torch.empty if n_boxes is None else torch.zeros
    transforms = new((B, 4), dtype=torch.float64, device=dev)
    glob = torch.empty(2, dtype=torch.float64, device=dev)
    boxes_out = new((B, 7), dtype=torch.float64, device=dev)
    attempt = new(B, dtype=torch.int32, device=dev)
    draws = new(4 + 8 * B, dtype=torch.int32, device=dev)
    seeds = (int(seed) & (2 ** 64 - 1), int(item) & 0xffffffff, int(epoch) & 0xffffffff)
    outs = (_lib.ptr(transforms) if B else None, _lib.ptr(glob), _lib.ptr(boxes_out) if B else None,
            _lib.ptr(attempt) if B else None, _lib.ptr(draws), _lib.current_stream())
    if n_boxes is None:
        _lib.check(_lib.load().lisec_augment_draw(_lib.ptr(boxes) if B else None, B, ctypes.byref(params), *seeds, *outs))
    else:
        _lib.check(_lib.load().lisec_augment_draw_n(_lib.ptr(boxes) if B else None, _int32_count(n_boxes), B,
                                                    ctypes.byref(params), *seeds, *outs))
    return transforms, glob, boxes_out, attempt, draws


def _point_args(points):
    """(address, dtype code, n, row stride) of device points (n, >= 3) float32 / float64 with unit element stride."""
    n = int(points.shape[0])
    if points.dtype not in (torch.float32, torch.float64):
        raise ValueError("points must be float32 or float64")
    if n and points.stride(1) != 1:
        raise ValueError("points need unit element stride")
    return (_lib.ptr(points) if n else None, 0 if points.dtype == torch.float32 else 1, n, int(points.stride(0)) if n else 3)


def augment_apply(points, boxes, transforms, glob, out, pad_limit, n_boxes=None):
    """lisec_augment_apply: device points (n, >= 3) float32 / float64 with unit element stride -> out (n, 3) dense, same dtype.
    n_boxes: a device int32 (1,) holding the number of box rows that count (lisec_augment_apply_n)."""
    n, B = int(points.shape[0]), int(boxes.shape[0])
    if points.dtype != out.dtype or points.dtype not in (torch.float32, torch.float64):
        raise ValueError("points and out must share one of float32 / float64")
    if n and (points.stride(1) != 1 or not out.is_contiguous() or tuple(out.shape) != (n, 3)):
        raise ValueError("points need unit element stride, out must be dense (n, 3)")
    tail = (_lib.ptr(transforms) if B else None, _lib.ptr(glob), float(pad_limit), _lib.ptr(out) if n else None,
            _lib.current_stream())
    if n_boxes is None:
        _lib.check(_lib.load().lisec_augment_apply(*_point_args(points), _lib.ptr(boxes) if B else None, B, *tail))
    else:
        _lib.check(_lib.load().lisec_augment_apply_n(*_point_args(points), _lib.ptr(boxes) if B else None,
                                                     _int32_count(n_boxes), B, *tail))
    return out


def augment_owner(points, boxes, pad_limit):
    """lisec_augment_owner: device points (n, >= 3), boxes (B, 7) float64 -> owner (n,) int32, the lowest box index holding
    each point, -1 for none and for pad rows."""
    n, B = int(points.shape[0]), int(boxes.shape[0])
    owner = torch.empty(n, dtype=torch.int32, device=points.device)
    _lib.check(_lib.load().lisec_augment_owner(*_point_args(points), _lib.ptr(boxes) if B else None, B, float(pad_limit),
                                               _lib.ptr(owner) if n else None, _lib.current_stream()))
    return owner


def augment_sample(boxes, db_boxes, db_offsets, n_samples, seed=0, item=0, epoch=0):
    """lisec_augment_sample: scene rows boxes (B, 7), the database's rows db_boxes (M, 7) and point offsets db_offsets
    (M + 1,) int32, K = n_samples candidates.  Returns device tensors (index (K,) int32, n_boxes (1,) int32, boxes_all
    (B + K, 7), point_offset (K + 1,) int32, draws (4 K,) uint32 held as int32 bits)."""
    B, M, K, dev = int(boxes.shape[0]), int(db_boxes.shape[0]), int(n_samples), boxes.device
    if db_offsets.dtype != torch.int32 or db_offsets.numel() != M + 1:
        raise ValueError("db_offsets must be int32 (M + 1,)")
    index = torch.empty(K, dtype=torch.int32, device=dev)
    n_boxes = torch.empty(1, dtype=torch.int32, device=dev)
    boxes_all = torch.empty((B + max(K, 0), 7), dtype=torch.float64, device=dev)
    point_offset = torch.empty(max(K, 0) + 1, dtype=torch.int32, device=dev)
    draws = torch.empty(4 * max(K, 0), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().lisec_augment_sample(_lib.ptr(boxes) if B else None, B, _lib.ptr(db_boxes) if M else None,
                                                _lib.ptr(db_offsets), M, K, int(seed) & (2 ** 64 - 1),
                                                int(item) & 0xffffffff, int(epoch) & 0xffffffff,
                                                _lib.ptr(index) if K else None, _lib.ptr(n_boxes),
                                                _lib.ptr(boxes_all) if B + K else None, _lib.ptr(point_offset),
                                                _lib.ptr(draws) if K else None, _lib.current_stream()))
    return index, n_boxes, boxes_all, point_offset, draws


def augment_paste(points, db_points, db_offsets, index, point_offset, boxes_all, n_boxes, out, pad_limit):
    """lisec_augment_paste: the scene points (n, >= 3) and the accepted objects of lisec_augment_sample -> out (cap, 3) dense
    in the points' dtype, which db_points (P, 3) shares: scene rows (those inside a pasted box as pad rows), the pasted
    points, pad rows up to cap."""
    n, K, cap = int(points.shape[0]), int(index.shape[0]), int(out.shape[0])
    B = int(boxes_all.shape[0]) - K
    if points.dtype != out.dtype or (db_points.numel() and db_points.dtype != out.dtype):
        raise ValueError("points, db_points and out must share one dtype")
    if not out.is_contiguous() or out.dim() != 2 or out.shape[1] != 3 or (db_points.numel() and not db_points.is_contiguous()):
        raise ValueError("out and db_points must be dense (rows, 3)")
    _lib.check(_lib.load().lisec_augment_paste(*_point_args(points), _lib.ptr(db_points) if db_points.numel() else None,
                                               _lib.ptr(db_offsets), _lib.ptr(index) if K else None, _lib.ptr(point_offset),
                                               _lib.ptr(boxes_all) if B + K else None, B, _int32_count(n_boxes), K,
                                               float(pad_limit), _lib.ptr(out) if cap else None, cap,
                                               _lib.current_stream()))
    return out
