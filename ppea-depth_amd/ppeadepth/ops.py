"""Autograd operators over the C ABI (include/ppea_depth.h).  Host glue only: every
forward/backward below is one (or two) kernel launches on the current HIP stream.

Reference call sites are cited per op (paths relative to /root/reference/ppeadepth/).
"""
import ctypes as _ct
import os
import weakref
from typing import NamedTuple as _NamedTuple, Optional

import torch
import torch.distributed as dist

from . import _abi
from ._abi import PpeaKernelError, call, ptr, stream_ptr, try_call
from .dist import log_collective

_F32 = torch.float32
_BF16 = torch.bfloat16

# bench.py sets this to a list; every k=31 launch then appends (kind, start_event, end_event)
# recorded on the launch stream (HIP events; the kernels run on torch's current stream).
PROFILE_DWCONV = None


PROFILE_REPLAY = {}       # kind -> closure re-issuing the first profiled launch of that kind (same arguments)


def _timed(kind, K, fn):
    if PROFILE_DWCONV is None or K != 31:
        return fn()
    PROFILE_REPLAY.setdefault(kind, fn)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    r = fn()
    e.record()
    PROFILE_DWCONV.append((kind, s, e))
    return r


def _suffix(t):
    if t.dtype == _F32:
        return "f32"
    if t.dtype == _BF16:
        return "bf16"
    raise _abi.PpeaKernelError(f"unsupported dtype {t.dtype}")


# ---------------------------------------------------------------------------------------------
# kernel-layout images of weights (packed filters, bf16 matrices), one cache for all of them
# ---------------------------------------------------------------------------------------------
_WEIGHT_IMAGES = {}


def _weight_image(w, tag, build, cache_trainable=False):
    """build(w), kept per weight OBJECT and `tag` (the kind of image).  An entry is keyed by the tensor object through a
    weak reference, not by its address (a freed weight's address can be handed to another model's weight), holds while
    the weight's version counter and shape are the recorded ones, and leaves with the weight.
    Policy: a trainable weight is updated by the flat Adam kernel through raw pointers, which does not bump the version
    counter, so the conv and depthwise packers build its image on every use (the pack launch is then part of the captured
    step as well).  `cache_trainable`: `_pw_matrices`, which is only ever given frozen 1x1 weights, caches what it gets."""
    if w.requires_grad and not cache_trainable:
        return build(w)
    key = (id(w), tag)
    hit = _WEIGHT_IMAGES.get(key)
    if hit is not None and hit[0]() is w and hit[1] == w._version and hit[2] == w.shape:
        return hit[3]
    image = build(w)
    _WEIGHT_IMAGES[key] = (weakref.ref(w, lambda _r: _WEIGHT_IMAGES.pop(key, None)), w._version, w.shape, image)
    return image


_MFMA_K = (31, 29, 27, 13)


def dwconv_lk_packed_supported(K):
    """The MFMA depthwise kernels (the ones that read a packed filter image) serve this kernel size."""
    return K in _MFMA_K


def pack_dwconv_filter(w, flip, out=None):
    """uint8 buffer with the bf16 Toeplitz source image of w [C,1,K,K] for the MFMA depthwise kernels (flip: the
    data-gradient image).  `out`: a buffer of an earlier call to rewrite in place (a captured graph keeps reading it)."""
    C, K = w.shape[0], w.shape[-1]
    if out is None:
        out = torch.empty(_abi.lib.ppea_dwconv_lk_packed_bytes(C, K), dtype=torch.uint8, device=w.device)
    wf = w.detach().to(_F32).contiguous()
    call("ppea_dwconv_lk_pack_bf16", ptr(wf), ptr(out), C, K, int(flip), stream_ptr())
    return out


def _packed_filter(w, flip):
    return _weight_image(w, ("dw", bool(flip)), lambda t: pack_dwconv_filter(t, flip))


def _mfma_ok(x, K, KS):
    return x.dtype == _BF16 and K in _MFMA_K and KS in (0, 5)


# ---------------------------------------------------------------------------------------------
# A1  large-kernel depthwise conv (+ fused 5x5 branch)   networks/replknet_adapter.py:151-168, 232-239
# ---------------------------------------------------------------------------------------------
class _DwConvLK(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_big, w_small, want_sums=False):
        x = x.contiguous()
        N, C, H, W = x.shape
        K = w_big.shape[-1]
        KS = 0 if w_small is None else w_small.shape[-1]
        wb = w_big.detach().to(_F32).contiguous()
        ws = None if w_small is None else w_small.detach().to(_F32).contiguous()
        y_big = torch.empty_like(x)
        y_small = torch.empty_like(x) if KS else None
        ctx.packed = None
        done = False
        sums = None
        if _mfma_ok(x, K, KS):
            pb = _packed_filter(w_big, False)
            ps = _packed_filter(w_small, False) if KS else None
            P = _abi.lib.ppea_dwconv_lk_stats_partials(N, C, H, W, K, KS) if (want_sums and KS) else 0
            if P > 0:
                # per-channel partial sums of both outputs from the conv's epilogue: the BatchNorm pair after it needs
                # no statistics pass (batchnorm.fused_bn_act(..., sums=(sums[0], sums[1])))
                sums = torch.empty(2, C, P, 2, device=x.device, dtype=_F32)
                done = _timed("fwd31", K, lambda: try_call(
                    "ppea_dwconv_lk_fwd_stats_bf16p", ptr(x), ptr(pb), ptr(ps), ptr(y_big), ptr(y_small), ptr(sums), N, C, H,
                    W, K, KS, stream_ptr()))
                if not done:
                    sums = None
            if not done:
                done = _timed("fwd31", K, lambda: try_call(
                    "ppea_dwconv_lk_fwd_bf16p", ptr(x), ptr(pb), ptr(ps), ptr(y_big), ptr(y_small), N, C, H, W, K, KS,
                    stream_ptr()))
            if done:
                ctx.packed = (w_big, w_small)
        if not done:
            _timed("fwd31", K, lambda: call(f"ppea_dwconv_lk_fwd_{_suffix(x)}", ptr(x), ptr(wb, _F32), ptr(ws),
                                             ptr(y_big), ptr(y_small), N, C, H, W, K, KS, stream_ptr()))
        ctx.save_for_backward(x, wb, ws)
        ctx.has_small = KS > 0
        ctx.w_dtypes = (w_big.dtype, None if w_small is None else w_small.dtype)
        if want_sums:
            if sums is not None:
                ctx.mark_non_differentiable(sums)
            return y_big, (y_small if KS else None), sums
        if KS:
            return y_big, y_small
        return y_big, None

    @staticmethod
    def backward(ctx, dy_big, dy_small, _dsums=None):
        x, wb, ws = ctx.saved_tensors
        N, C, H, W = x.shape
        K = wb.shape[-1]
        KS = ws.shape[-1] if ctx.has_small else 0
        dx = dwb = dws = None
        if dy_big is None:
            dy_big = torch.zeros_like(x)
        dy_big = dy_big.contiguous().to(x.dtype)
        if ctx.has_small:
            dy_small = (torch.zeros_like(x) if dy_small is None else dy_small.contiguous().to(x.dtype))
        else:
            dy_small = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            done = False
            if ctx.packed is not None:
                pb = _packed_filter(ctx.packed[0], True)
                ps = _packed_filter(ctx.packed[1], True) if KS else None
                done = _timed("bwd31", K, lambda: try_call(
                    "ppea_dwconv_lk_bwd_data_bf16p", ptr(dy_big), ptr(dy_small), ptr(pb), ptr(ps), ptr(dx), N, C, H, W, K, KS,
                    stream_ptr()))
            if not done:
                _timed("bwd31", K, lambda: call(f"ppea_dwconv_lk_bwd_data_{_suffix(x)}", ptr(dy_big),
                                                 ptr(dy_small), ptr(wb), ptr(ws), ptr(dx), N, C, H, W, K, KS,
                                                 stream_ptr()))
        want_b, want_s = ctx.needs_input_grad[1], ctx.has_small and ctx.needs_input_grad[2]
        if want_b and _mfma_ok(x, K, KS):
            # bf16 activations: both filter gradients from one MFMA launch that reads x once (csrc/dwconv_wgrad.hip)
            got = dwconv_lk_bwd_filter(x, dy_big, dy_small if want_s else None, K)
            if got is not None:
                dwb = got[0].view_as(wb).to(ctx.w_dtypes[0])
                if want_s:
                    dws = got[1].view_as(ws).to(ctx.w_dtypes[1])
                want_b = want_s = False
        if want_b or want_s:
            # (the fp32 copies are held in locals: a temporary freed before the next allocation would hand its block on)
            xf = x.float().contiguous()
        if want_b:
            dwb, dyf = torch.empty_like(wb), dy_big.float().contiguous()
            call("ppea_dwconv_lk_bwd_filter_f32", ptr(xf), ptr(dyf), ptr(dwb), N, C, H, W, K, stream_ptr())
            dwb = dwb.to(ctx.w_dtypes[0])
        if want_s:
            dws, dyf = torch.empty_like(ws), dy_small.float().contiguous()
            call("ppea_dwconv_lk_bwd_filter_f32", ptr(xf), ptr(dyf), ptr(dws), N, C, H, W, KS, stream_ptr())
            dws = dws.to(ctx.w_dtypes[1])
        return dx, dwb, dws, None


class _DwConvLKBn(torch.autograd.Function):
    """(DW_k(t), DW_5(t)) with t = relu(BN(z)) never materialised: the BatchNorm of RepLKBlock's pw1 (training mode,
    statistics from the producing 1x1 conv's epilogue `sums`) and its ReLU are applied while the depthwise kernel stages its
    planes (csrc/dwconv_mfma.hip, BnIn).  Backward: depthwise data gradient, then the BatchNorm + ReLU backward kernels on
    the saved pre-BN tensor (relu' is recomputed from it).   networks/replknet_adapter.py:305-308, 182-197, 232-239"""

    @staticmethod
    def forward(ctx, z, sums, gamma, beta, rm, rv, eps, momentum, w_big, w_small):
        z = z.contiguous()
        N, C, H, W = z.shape
        K = w_big.shape[-1]
        pb, ps = _packed_filter(w_big, False), _packed_filter(w_small, False)
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        st = torch.empty(2, C, device=z.device, dtype=_F32)                     # mean | invstd
        y_big, y_small = torch.empty_like(z), torch.empty_like(z)
        _timed("fwd31", K, lambda: call(
            "ppea_dwconv_lk_fwd_bn_bf16p", ptr(z), ptr(pb), ptr(ps), ptr(y_big), ptr(y_small), ptr(sums, _F32), sums.shape[1],
            N * H * W, ptr(g), ptr(b), float(eps), float(momentum), ptr(rm), ptr(rv), ptr(st[0]), ptr(st[1]), N, C, H, W, K, 5,
            stream_ptr()))
        ctx.save_for_backward(z, st, g, b)
        ctx.packed = (w_big, w_small)
        ctx.pdt = (gamma.dtype, beta.dtype)
        ctx.mark_non_differentiable(st)
        ctx.set_materialize_grads(False)
        return y_big, y_small, st

    @staticmethod
    def backward(ctx, dy_big, dy_small, _dst):
        z, st, g, b = ctx.saved_tensors
        N, C, H, W = z.shape
        K = ctx.packed[0].shape[-1]
        dy_big = torch.zeros_like(z) if dy_big is None else dy_big.contiguous().to(z.dtype)
        dy_small = torch.zeros_like(z) if dy_small is None else dy_small.contiguous().to(z.dtype)
        dt = torch.empty_like(z)
        pb, ps = _packed_filter(ctx.packed[0], True), _packed_filter(ctx.packed[1], True)
        _timed("bwd31", K, lambda: call("ppea_dwconv_lk_bwd_data_bf16p", ptr(dy_big), ptr(dy_small), ptr(pb), ptr(ps),
                                        ptr(dt), N, C, H, W, K, 5, stream_ptr()))
        # BatchNorm + ReLU backward on the saved pre-BN tensor (as _BnActChannel / _BnAct would)
        HW = H * W
        stats = _ptr_array((st[0], st[1], g, b, None, None, None, None))
        dz = torch.empty_like(z)
        sfx = _suffix(z)
        if bn_channel_ok(z):
            sums = torch.empty(3, C, device=z.device, dtype=_F32)
            call(f"ppea_bn_bwd_channel_{sfx}", ptr(dt), ptr(z), None, stats, None, 1.0 / float(N * HW), None, ptr(dz), None,
                 ptr(sums), ACT_RELU, N, C, HW, stream_ptr())
        else:
            sums, _, _ = _bn_bwd_sums(dt, z, None, stats, None, ACT_RELU)
            call(f"ppea_bn_bwd_apply_{sfx}", ptr(dt), ptr(z), None, stats, None, ptr(sums), 1.0 / float(N * HW), ptr(dz), None,
                 ACT_RELU, N, C, HW, stream_ptr())
        dg = sums[1].to(ctx.pdt[0]) if ctx.needs_input_grad[2] else None
        db = sums[0].to(ctx.pdt[1]) if ctx.needs_input_grad[3] else None
        return dz, None, dg, db, None, None, None, None, None, None


def dwconv_lk_bwd_filter(x, dy_big, dy_small, K):
    """(dw_big [C,K,K], dw_small [C,5,5] or None) fp32: the filter gradients of the depthwise pair for bf16 x / dy
    [N,C,H,W] from one launch on the matrix cores + a fixed-order sum of its (n, row band) parts; None where the kernel
    does not serve (K, KS) -- the caller then keeps ppea_dwconv_lk_bwd_filter_f32."""
    N, C, H, W = x.shape
    KS = 0 if dy_small is None else 5
    nbytes = _abi.lib.ppea_dwconv_lk_bwd_filter_workspace_bytes(N, C, H, W, K, KS)
    if nbytes < 0:
        return None
    ws = torch.empty(nbytes // 4, device=x.device, dtype=_F32)
    dwb = torch.empty(C, K, K, device=x.device, dtype=_F32)
    dws = torch.empty(C, 5, 5, device=x.device, dtype=_F32) if KS else None
    if not try_call("ppea_dwconv_lk_bwd_filter_bf16", ptr(x, _BF16), ptr(dy_big, _BF16), ptr(dy_small, _BF16), ptr(dwb),
                    ptr(dws), ptr(ws), N, C, H, W, K, KS, stream_ptr()):
        return None
    return dwb, dws


def dwconv_lk_bn_supported(shape, K, KS):
    """The fused form needs the MFMA depthwise kernel (bf16 input of `shape`, k in 31/29/27/13, 5x5 branch) and a shape
    that kernel serves."""
    N, C, H, W = shape
    return K in _MFMA_K and KS == 5 and _abi.lib.ppea_dwconv_lk_stats_partials(N, C, H, W, K, KS) > 0


def dwconv_lk_bn(z, sums, bn, w_big, w_small):
    """-> (DW_k(relu(BN(z))), DW_5(relu(BN(z))), stats [2,C] = mean | invstd).  `sums`: the partial sums the 1x1 conv that
    produced z left (pwconv_frozen(..., want_sums=True)).  Frozen depthwise filters only; updates bn's running statistics."""
    # (the filters are passed as they are: the packed fragment images are cached per weight OBJECT)
    assert not w_big.requires_grad and not w_small.requires_grad
    return _DwConvLKBn.apply(z, sums, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum,
                             w_big, w_small)


def dwconv_lk(x, w_big, w_small=None, want_sums=False):
    """(DW_k(x), DW_ks(x)) with stride 1 / pad k//2 / no bias; second is None without w_small.
    want_sums: -> (y_big, y_small, sums [2, C, P, 2] or None): per-channel partial (sum, sum of squares) of both outputs
    from the conv's epilogue, for the two BatchNorms that follow."""
    if want_sums:
        return _DwConvLK.apply(x, w_big, w_small, True)
    return _DwConvLK.apply(x, w_big, w_small)


# ---------------------------------------------------------------------------------------------
# A18+A19  BackprojectDepth -> Project3D                         layers.py:138-199
# ---------------------------------------------------------------------------------------------
def _device_f32(name, *ts):
    """fp32 contiguous views of device tensors; a host tensor is refused (no CPU path behind an op)."""
    for t in ts:
        if not t.is_cuda:
            raise PpeaKernelError(f"{name}: PPEA-Depth HIP kernels need tensors on a HIP device (no CPU fallback)")
    return [t.contiguous().float() for t in ts]


def _bwd_workspace(op, like, H, W):
    """The per-block partial sums of `ppea_<op>_bwd_f32` for like.shape[0] images of H x W, sized by the library."""
    nbytes = getattr(_abi.lib, f"ppea_{op}_bwd_workspace_bytes")(like.shape[0], H, W)
    return torch.empty(nbytes // 4, device=like.device, dtype=_F32)


class _BackprojectProject(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, inv_K, P, eps):
        depth, inv_K, P = _device_f32("backproject_project", depth, inv_K, P)
        B, _, H, W = depth.shape
        grid = torch.empty(B, H, W, 2, device=depth.device, dtype=_F32)
        call("ppea_backproject_project_fwd_f32", ptr(depth), ptr(inv_K), ptr(P), ptr(grid), B, H, W,
             float(eps), stream_ptr())
        ctx.save_for_backward(depth, inv_K, P)
        ctx.eps = float(eps)
        return grid

    @staticmethod
    def backward(ctx, d_grid):
        depth, inv_K, P = ctx.saved_tensors
        B, _, H, W = depth.shape
        d_depth = torch.empty_like(depth)
        dP = torch.empty_like(P)
        ws = _bwd_workspace("backproject_project", depth, H, W)
        call("ppea_backproject_project_bwd_f32", ptr(depth), ptr(inv_K), ptr(P),
             ptr(d_grid.contiguous().float()), ptr(d_depth), ptr(dP), ptr(ws), B, H, W, ctx.eps, stream_ptr())
        return d_depth, None, dP, None


def backproject_project(depth, inv_K, K, T, eps=1e-7):
    """depth [B,1,H,W] -> sampling grid [B,H,W,2];  P = (K @ T)[:, :3] keeps the pose gradient."""
    P = torch.matmul(K, T)[:, :3, :]
    return _BackprojectProject.apply(depth, inv_K, P, eps)


# The two halves on their own (layers.BackprojectDepth / layers.Project3D): the same arithmetic split at the point cloud.
def _per_item(m, B):
    """[1,4,4] -> [B,4,4] as the kernels index it (one small copy; autograd sums the gradient back); [B,4,4] as it is."""
    return m if m.shape[0] == B else m.expand(B, 4, 4).contiguous()


class _Backproject(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, inv_K):
        B, _, H, W = depth.shape
        points = torch.empty(B, 4, H * W, device=depth.device, dtype=_F32)
        call("ppea_backproject_fwd_f32", ptr(depth), ptr(inv_K), ptr(points), B, H, W, stream_ptr())
        ctx.save_for_backward(depth, inv_K)
        return points

    @staticmethod
    def backward(ctx, d_points):
        depth, inv_K = ctx.saved_tensors
        B, _, H, W = depth.shape
        d_depth = torch.empty_like(depth) if ctx.needs_input_grad[0] else None
        d_inv_K = ws = None
        if ctx.needs_input_grad[1]:
            d_inv_K = torch.empty_like(inv_K)
            ws = _bwd_workspace("backproject", depth, H, W)
        call("ppea_backproject_bwd_f32", ptr(depth), ptr(inv_K), ptr(d_points.contiguous().float()), ptr(d_depth),
             ptr(d_inv_K), ptr(ws), B, H, W, stream_ptr())
        return d_depth, d_inv_K


def backproject(depth, inv_K):
    """depth [B,1,H,W], inv_K [B,4,4] -> homogeneous points [B,4,HW] fp32 (row 3 = 1), one launch; fp32 under autocast.
    inv_K [1,4,4] serves every item, as it does in the composite's broadcasting matmul (the reference's matching encoders
    back-project D depth planes with one camera); its gradient is then the sum over the items."""
    depth, inv_K = _device_f32("backproject", depth, inv_K)
    B = depth.shape[0]
    if depth.dim() != 4 or depth.shape[1] != 1 or inv_K.dim() != 3 or inv_K.shape[0] not in (1, B) or inv_K.shape[1:] != (4, 4):
        raise PpeaKernelError(f"backproject: depth {tuple(depth.shape)}, inv_K {tuple(inv_K.shape)}")
    with torch.autocast("cuda", enabled=False):
        return _Backproject.apply(depth, _per_item(inv_K, B))


class _Project3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, P, H, W, eps, with_depth):
        B = points.shape[0]
        grid = torch.empty(B, H, W, 2, device=points.device, dtype=_F32)
        z = torch.empty(B, 1, H, W, device=points.device, dtype=_F32) if with_depth else None
        call("ppea_project3d_fwd_f32", ptr(points), ptr(P), ptr(grid), ptr(z), B, H, W, float(eps), stream_ptr())
        ctx.save_for_backward(points, P)
        ctx.set_materialize_grads(False)         # an unused output of the (grid, z) pair costs no zero fill
        ctx.dims = (H, W, float(eps), with_depth)
        return (grid, z) if with_depth else grid

    @staticmethod
    def backward(ctx, d_grid, d_z=None):
        points, P = ctx.saved_tensors
        H, W, eps, with_depth = ctx.dims
        B = points.shape[0]
        want_points, want_P = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if d_grid is None and d_z is None:
            return (None,) * 6
        if d_grid is None:                       # only the projected depth was used downstream
            d_grid = torch.zeros(B, H, W, 2, device=points.device, dtype=_F32)
        if d_z is not None:
            d_z = d_z.contiguous().float()
        d_points = torch.empty_like(points) if want_points else None
        dP = ws = None
        if want_P:
            dP = torch.empty_like(P)
            ws = _bwd_workspace("project3d", points, H, W)
        call("ppea_project3d_bwd_f32", ptr(points), ptr(P), ptr(d_grid.contiguous().float()), ptr(d_z), ptr(d_points),
             ptr(dP), ptr(ws), B, H, W, eps, stream_ptr())
        return d_points, dP, None, None, None, None


def project3d(points, K, T, H, W, eps=1e-7, with_depth=False):
    """points [B,4,HW] (row 3 need not be 1), K, T [B,4,4] -> sampling grid [B,H,W,2] fp32, and with `with_depth` the
    projected depth cam[2] as [B,1,H,W] (Project3D's `dc=True` pair).  K @ T is one 4x4 product as in
    `backproject_project` and hands K and T their gradients; the kernels read its rows 0-2 in place (no copy of the
    `[:, :3, :]` slice, no padding of its gradient).  K and T may each be [1,4,4] for all items, as in the composite's
    broadcasting matmul: the product is still formed once.  fp32 under autocast."""
    points, K, T = _device_f32("project3d", points, K, T)
    B = points.shape[0]
    if tuple(points.shape) != (B, 4, H * W) or any(m.dim() != 3 or m.shape[0] not in (1, B) or m.shape[1:] != (4, 4)
                                                   for m in (K, T)):
        raise PpeaKernelError(f"project3d: points {tuple(points.shape)}, K {tuple(K.shape)}, T {tuple(T.shape)} "
                              f"for {H} x {W}")
    with torch.autocast("cuda", enabled=False):
        return _Project3D.apply(points, _per_item(torch.matmul(K, T), B), int(H), int(W), eps, bool(with_depth))


# ---------------------------------------------------------------------------------------------
# A20  grid_sample (bilinear, align_corners=True)            trainer.py:911-914, rkm.py:299
# ---------------------------------------------------------------------------------------------
class _GridSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, grid, padding):
        src = src.contiguous().float()
        grid = grid.contiguous().float()
        B, C, Hi, Wi = src.shape
        _, Ho, Wo, _ = grid.shape
        out = torch.empty(B, C, Ho, Wo, device=src.device, dtype=_F32)
        call("ppea_grid_sample_fwd_f32", ptr(src), ptr(grid), ptr(out), B, C, Hi, Wi, Ho, Wo, padding,
             stream_ptr())
        ctx.save_for_backward(src, grid)
        ctx.padding = padding
        return out

    @staticmethod
    def backward(ctx, d_out):
        src, grid = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            raise _abi.PpeaKernelError("grid_sample: gradient w.r.t. the source image is not part of the "
                                       "hot path (sources are input frames)")
        B, C, Hi, Wi = src.shape
        _, Ho, Wo, _ = grid.shape
        d_grid = torch.empty_like(grid)
        call("ppea_grid_sample_bwd_grid_f32", ptr(src), ptr(grid), ptr(d_out.contiguous().float()),
             ptr(d_grid), B, C, Hi, Wi, Ho, Wo, ctx.padding, stream_ptr())
        return None, d_grid, None


def grid_sample(src, grid, padding_mode="border"):
    return _GridSample.apply(src, grid, {"zeros": 0, "border": 1}[padding_mode])


# ---------------------------------------------------------------------------------------------
# A21+A22  reprojection loss                             trainer.py:995-1007, layers.py:226-257
# ---------------------------------------------------------------------------------------------
class _SsimL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, alpha):
        pred = pred.contiguous().float()
        target = target.contiguous().float()
        B, C, H, W = pred.shape
        out = torch.empty(B, 1, H, W, device=pred.device, dtype=_F32)
        call("ppea_ssim_l1_fwd_f32", ptr(pred), ptr(target), ptr(out), H * W, B, C, H, W, float(alpha),
             stream_ptr())
        ctx.save_for_backward(pred, target)
        ctx.alpha = float(alpha)
        return out

    @staticmethod
    def backward(ctx, d_out):
        pred, target = ctx.saved_tensors
        B, C, H, W = pred.shape
        d_pred = torch.empty_like(pred)
        call("ppea_ssim_l1_bwd_f32", ptr(pred), ptr(target), ptr(d_out.contiguous().float()), H * W,
             ptr(d_pred), B, C, H, W, ctx.alpha, stream_ptr())
        return d_pred, None, None


def ssim_l1(pred, target, alpha=0.85):
    """alpha * mean_C SSIM(pred, target) + (1-alpha) * mean_C |target - pred| -> [B,1,H,W].
    Differentiable w.r.t. pred only (target is an input frame)."""
    return _SsimL1.apply(pred, target, alpha)


# ---------------------------------------------------------------------------------------------
# A23  edge-aware smoothness                                         layers.py:210-223
# ---------------------------------------------------------------------------------------------
class _SmoothLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, img):
        disp = disp.contiguous().float()
        img = img.contiguous().float()
        B, C, H, W = img.shape
        nb = _abi.lib.ppea_smooth_num_partials()
        partials = torch.empty(nb, 2, device=disp.device, dtype=_F32)
        call("ppea_smooth_fwd_f32", ptr(disp), ptr(img), ptr(partials), B, C, H, W, stream_ptr())
        s = partials.sum(0)
        ctx.save_for_backward(disp, img)
        ctx.nx = float(B * H * (W - 1))
        ctx.ny = float(B * (H - 1) * W)
        return s[0] / ctx.nx + s[1] / ctx.ny

    @staticmethod
    def backward(ctx, g):
        disp, img = ctx.saved_tensors
        B, C, H, W = img.shape
        d_disp = torch.empty_like(disp)
        call("ppea_smooth_bwd_f32", ptr(disp), ptr(img), 1.0 / ctx.nx, 1.0 / ctx.ny, ptr(d_disp), B, C, H, W,
             stream_ptr())
        return d_disp * g, None      # upstream scalar stays on the device (no host sync)


def smooth_loss(disp, img):
    return _SmoothLoss.apply(disp, img)


# ---------------------------------------------------------------------------------------------
# A24/A25  per-pixel selection                                     trainer.py:1069-1091
# ---------------------------------------------------------------------------------------------
class _LossSelect(torch.autograd.Function):
    """S = reproj.shape[1] source frames, S in {1, 2} (ppea_loss_select_f32)."""

    @staticmethod
    def forward(ctx, reproj, identity, noise, selec, *warped):
        reproj = reproj.contiguous().float()
        B, S, H, W = reproj.shape
        dev = reproj.device
        warped = [w.contiguous().float() for w in warped]
        sel = torch.empty(B, 1, H, W, device=dev, dtype=_F32)
        src = torch.empty(B, 1, H, W, device=dev, dtype=torch.uint8)
        fidx = torch.empty(B, 1, H, W, device=dev, dtype=torch.int64)
        aidx = torch.empty(B, 1, H, W, device=dev, dtype=torch.int64)
        call("ppea_loss_select_f32", ptr(reproj), ptr(identity.contiguous().float()),
             ptr(warped[0] if warped else None), ptr(warped[1] if warped else None),
             ptr(None if noise is None else noise.contiguous().float()), ptr(sel), ptr(src), ptr(fidx),
             ptr(aidx), B, S, warped[0].shape[1] if warped else 0, H, W, int(bool(selec)), stream_ptr())
        ctx.save_for_backward(src)
        ctx.n_src = S
        ctx.mark_non_differentiable(src, fidx, aidx)
        ctx.set_materialize_grads(False)
        return sel, src, fidx, aidx

    @staticmethod
    def backward(ctx, d_sel, _a, _b, _c):
        (src,) = ctx.saved_tensors
        d = None
        if d_sel is not None:
            d = torch.cat([d_sel * (src == c) for c in range(ctx.n_src)], 1)
        return (d,) + (None,) * (len(ctx.needs_input_grad) - 1)


def loss_select(reproj, identity, warped, noise, selec_reproj):
    """-> (selected reprojection loss [B,1,H,W], source idx u8, frame argmin i64, automask argmin i64) for S =
    reproj.shape[1] source frames, S in {1, 2}; `identity` [B,S,H,W]; `warped`: the S warped frames, read for
    `selec_reproj` only, or None.  One frame (frame_ids [0, -1]): the selected loss is that frame's, the source and frame
    indices are 0, and `selec_reproj` -- which falls back on the OTHER frame -- is refused."""
    S = reproj.shape[1]
    if S not in (1, 2) or identity.shape[1] != S:
        raise ValueError(f"loss_select: reproj {tuple(reproj.shape)}, identity {tuple(identity.shape)}: one or two source "
                         "frames, the same in both")
    if selec_reproj and S == 1:
        raise ValueError("loss_select: selec_reproj needs two source frames (train frame_ids [0, -1] with --selec_reproj, "
                         "which switches it off)")
    if selec_reproj and (warped is None or len(warped) != S):
        raise ValueError("loss_select: selec_reproj reads the warped frame of every source frame")
    return _LossSelect.apply(reproj, identity, noise, selec_reproj, *(warped if selec_reproj else ()))


class _LossTail(torch.autograd.Function):
    """Tail of compute_losses (trainer.py:1092-1139) in one pass per direction (csrc/photometric.hip loss_tail_*):
    -> (rl, consistency_loss, mask, consistency_target).  `reproj` [B,S,H,W], S in {1, 2}, is the differentiable input the
    selected loss `sel` was taken from (`src`: which channel, 2 = forced zero); its gradient is produced directly."""

    @staticmethod
    def forward(ctx, reproj, sel, src, auto_idx, cons, aug, multi, mono, is_multi):
        B, _, H, W = sel.shape
        dev = sel.device
        sel = sel.contiguous().float()
        mask = torch.empty(B, 1, H, W, device=dev, dtype=_F32)
        target = torch.empty(B, 1, H, W, device=dev, dtype=_F32) if is_multi else None
        nblk = _abi.lib.ppea_loss_tail_blocks(B * H * W)
        partial = torch.empty(nblk * 3, device=dev, dtype=_F32)
        out = torch.empty(3, device=dev, dtype=_F32)
        multi_c = None if multi is None else multi.detach().contiguous().float()
        mono_c = None if mono is None else mono.detach().contiguous().float()
        call("ppea_loss_tail_fwd_f32", ptr(sel), ptr(auto_idx), ptr(None if cons is None else cons.contiguous().float()),
             ptr(None if aug is None else aug.reshape(-1).contiguous().float()), ptr(multi_c), ptr(mono_c), ptr(mask),
             ptr(target), ptr(partial), ptr(out), B, H, W, int(bool(is_multi)), stream_ptr())
        ctx.save_for_backward(mask, src, out, multi_c, mono_c)
        ctx.dims = (B, H, W, bool(is_multi), multi is not None and multi.requires_grad)
        ctx.n_src = int(reproj.shape[1])                     # source frames: d_reproj [B,S,H,W]
        ctx.set_materialize_grads(False)
        rl, cl = out[0], out[1]
        if target is not None:
            ctx.mark_non_differentiable(mask, target)
            return rl, cl, mask, target
        ctx.mark_non_differentiable(mask)
        return rl, cl, mask

    @staticmethod
    def backward(ctx, g_rl, g_cl, *_unused):
        mask, src, out, multi, mono = ctx.saved_tensors
        B, H, W, is_multi, multi_grad = ctx.dims
        dev = mask.device
        d_reproj = torch.empty(B, ctx.n_src, H, W, device=dev, dtype=_F32) if ctx.needs_input_grad[0] else None
        d_multi = torch.empty(B, 1, H, W, device=dev, dtype=_F32) if (is_multi and multi_grad and g_cl is not None) else None
        call("ppea_loss_tail_bwd_f32", ptr(mask), ptr(src), ptr(out), ptr(None if g_rl is None else g_rl.contiguous().float()),
             ptr(None if g_cl is None else g_cl.contiguous().float()), ptr(multi), ptr(mono), ptr(d_reproj), ptr(d_multi),
             B, ctx.n_src, H, W, stream_ptr())
        return d_reproj, None, None, None, None, None, d_multi, None, None


def loss_tail(reproj, sel, src, auto_idx=None, cons=None, aug=None, multi=None, mono=None, is_multi=False):
    return _LossTail.apply(reproj, sel, src, auto_idx, cons, aug, multi, mono, is_multi)


# ---------------------------------------------------------------------------------------------
# A9/A10  cost volume (runs under no_grad in the reference, rkm.py:427)
# ---------------------------------------------------------------------------------------------
CV_BF16 = True      # bf16 features on the packed-pair form of the kernel (False: widened to fp32 first; bit-identical results)
CV_MAX_FRAMES = 4      # up to three past frames plus the future one


def cost_volume(cur, lookup, poses, K, inv_K, bins, eps=1e-7):
    """One lookup frame: cur, lookup [B,C,h,w]; poses [B,4,4] (zeroed pose = skipped item); -> raw cost [B,D,h,w]."""
    return cost_volume_multi(cur, lookup[:, None], poses[:, None], K, inv_K, bins, eps)


@torch.no_grad()
def cost_volume_multi(cur, lookups, poses, K, inv_K, bins, eps=1e-7):
    """cur [B,C,h,w]; lookups [B,F,C,h,w]; poses [B,F,4,4] (a zeroed pose = that frame of that item skipped);
    -> raw cost [B,D,h,w] averaged over the frames that contribute at each (bin, pixel), in ONE launch."""
    B, F, C, h, w = lookups.shape
    if F > CV_MAX_FRAMES:
        raise _abi.PpeaKernelError(f"cost_volume_multi serves 1 .. {CV_MAX_FRAMES} lookup frames, got {F}")
    D = bins.shape[0]
    P = torch.matmul(K[:, None], poses)[:, :, :3, :].contiguous().float()
    skip = (poses.reshape(B, F, -1).sum(2) == 0).to(torch.int32)
    cost = torch.empty(B, D, h, w, device=cur.device, dtype=_F32)
    inv_K, bins = inv_K.contiguous().float(), bins.contiguous().float()
    tail = (ptr(P), ptr(inv_K), ptr(bins), ptr(skip), ptr(cost), B, F, C, h, w, D, float(eps), stream_ptr())
    if CV_BF16 and cur.dtype == _BF16 and lookups.dtype == _BF16 and C % 2 == 0:
        # channel pairs packed into dwords (half the bytes through the L1), same arithmetic
        cur, lookups = cur.contiguous(), lookups.contiguous()
        pairs = torch.empty((1 + F) * B * (C // 2) * h * w, device=cur.device, dtype=torch.int32)
        call("ppea_cost_volume_multi_fwd_bf16", ptr(cur), ptr(lookups), ptr(pairs), *tail)
        return cost
    cur, lookups = cur.contiguous().float(), lookups.contiguous().float()
    call("ppea_cost_volume_multi_fwd_f32", ptr(cur), ptr(lookups), *tail)
    return cost


@torch.no_grad()
def cost_volume_reduce(cost, bins):
    """-> (masked cost [B,D,h,w], confidence [B,h,w], argmin int64 [B,h,w], lowest-cost 1/depth [B,h,w])."""
    B, D, h, w = cost.shape
    dev = cost.device
    out = torch.empty_like(cost)
    conf = torch.empty(B, h, w, device=dev, dtype=_F32)
    idx = torch.empty(B, h, w, device=dev, dtype=torch.int64)
    low = torch.empty(B, h, w, device=dev, dtype=_F32)
    call("ppea_cost_volume_reduce_f32", ptr(cost.contiguous()), ptr(bins.contiguous().float()), ptr(out),
         ptr(conf), ptr(idx), ptr(low), B, D, h, w, stream_ptr())
    return out, conf, idx, low


# ---- video streaming: the lookups are the last F frames, kept in a device ring (inference.DepthStream) ----------------
# `state`: a stream's counters on the device, int32 [1 + B]: [0] the head slot, [1 + b] the frames item b has seen since its
# reset (clamped at F).  The ring kernels read them; nothing reads them on the host.
def _ring_dims(ring, state):
    F, B = ring.shape[:2]
    if not 1 <= F <= CV_MAX_FRAMES:
        raise _abi.PpeaKernelError(f"a feature ring holds 1 .. {CV_MAX_FRAMES} frames, got {F}")
    if state is not None and (state.dtype != torch.int32 or state.shape != (1 + B,) or state.device != ring.device):
        raise _abi.PpeaKernelError(f"stream state must be int32 [1 + {B}] on {ring.device}")
    if ring.dtype not in (_F32, torch.int32):
        raise _abi.PpeaKernelError(f"a feature ring is fp32 or int32 channel pairs, got {ring.dtype}")
    return F, B


@torch.no_grad()
def pack_pairs(x):
    """bf16 [B,C,h,w], C even -> the plane sweep's channel-pair dwords, int32 [B,C/2,h,w] (cv_pack_pairs layout)."""
    B, C, h, w = x.shape
    if x.dtype != _BF16 or C % 2:
        raise _abi.PpeaKernelError(f"pack_pairs takes bf16 maps with an even channel count, got {x.dtype} C = {C}")
    out = torch.empty(B, C // 2, h, w, device=x.device, dtype=torch.int32)
    call("ppea_cv_ring_store_bf16", ptr(x.contiguous()), ptr(out), None, B, 1, C, h, w, stream_ptr())
    return out


@torch.no_grad()
def ring_store(x, ring, state):
    """x [B,C,h,w] into the slot the device-side head names: fp32 into an fp32 ring [F,B,C,h,w], bf16 as channel pairs into
    an int32 ring [F,B,C/2,h,w]."""
    F, B = _ring_dims(ring, state)
    C, h, w = x.shape[1:]
    if ring.dtype == _F32:
        if x.dtype != _F32 or tuple(ring.shape[1:]) != tuple(x.shape):
            raise _abi.PpeaKernelError(f"ring_store: {x.dtype} {tuple(x.shape)} into an fp32 ring {tuple(ring.shape)}")
        call("ppea_cv_ring_store_f32", ptr(x.contiguous()), ptr(ring), ptr(state), B, F, C, h, w, stream_ptr())
    else:
        if x.dtype != _BF16 or C % 2 or tuple(ring.shape[1:]) != (x.shape[0], C // 2, h, w):
            raise _abi.PpeaKernelError(f"ring_store: {x.dtype} {tuple(x.shape)} into a pair ring {tuple(ring.shape)}")
        call("ppea_cv_ring_store_bf16", ptr(x.contiguous()), ptr(ring), ptr(state), B, F, C, h, w, stream_ptr())
    return ring


@torch.no_grad()
def ring_advance(state, F):
    """A frame has been pushed: head <- (head + 1) mod F, seen <- min(seen + 1, F).  Call it after the sweep and the store."""
    call("ppea_cv_ring_advance", ptr(state, torch.int32), state.shape[0] - 1, int(F), stream_ptr())
    return state


@torch.no_grad()
def cost_volume_ring(cur, ring, state, poses, K, inv_K, bins, eps=1e-7, zero_pose_skip=True):
    """`cost_volume_multi` with lookup frame f of item b read from slot (head - 1 - f) mod F of `ring` (`ring_store`'s
    layout); a frame is skipped where seen[b] <= f or, with `zero_pose_skip`, where its pose is zeroed.  cur: fp32 [B,C,h,w]
    for an fp32 ring; bf16 [B,C,h,w] (packed here, one launch) or already packed int32 [B,C/2,h,w] for a pair ring.  Same
    bits as `cost_volume_multi` on the frames gathered in order.  (`zero_pose_skip=False`: the caller's poses are zero exactly
    where seen says so, e.g. `pose_chain_ring`'s -- three small launches less.)"""
    F, B = _ring_dims(ring, state)
    if state is None:
        raise _abi.PpeaKernelError("cost_volume_ring needs the stream state")
    D = bins.shape[0]
    if tuple(poses.shape) != (B, F, 4, 4):
        raise _abi.PpeaKernelError(f"cost_volume_ring: poses {tuple(poses.shape)} for a ring of {F} frames, B = {B}")
    P = torch.matmul(K[:, None], poses)[:, :, :3, :].contiguous().float()
    skip = (poses.reshape(B, F, -1).sum(2) == 0).to(torch.int32) if zero_pose_skip else None
    inv_K, bins = inv_K.contiguous().float(), bins.contiguous().float()
    if ring.dtype == _F32:
        C, h, w = ring.shape[2:]
        if cur.dtype != _F32 or tuple(cur.shape) != (B, C, h, w):
            raise _abi.PpeaKernelError(f"cost_volume_ring: cur {cur.dtype} {tuple(cur.shape)}, fp32 ring {tuple(ring.shape)}")
        name = "ppea_cost_volume_ring_fwd_f32"
    else:
        if cur.dtype == _BF16:
            cur = pack_pairs(cur)
        C, h, w = 2 * ring.shape[2], ring.shape[3], ring.shape[4]
        if cur.dtype != torch.int32 or tuple(cur.shape) != (B, C // 2, h, w):
            raise _abi.PpeaKernelError(f"cost_volume_ring: cur {cur.dtype} {tuple(cur.shape)}, pair ring {tuple(ring.shape)}")
        name = "ppea_cost_volume_ring_fwd_bf16"
    cost = torch.empty(B, D, h, w, device=ring.device, dtype=_F32)
    call(name, ptr(cur.contiguous()), ptr(ring), ptr(state), ptr(P), ptr(inv_K), ptr(bins), ptr(skip), ptr(cost), B, F, C, h,
         w, D, float(eps), stream_ptr())
    return cost


# ---------------------------------------------------------------------------------------------
# Validation metric (trainer.py:780-843, and val_ddad's, :583-623): the per-image error protocol on the device   (csrc/eval_metrics.hip)
# ---------------------------------------------------------------------------------------------
# any other split name ("ddad" and "benchmark" among them): the 80 m range test only (mode 0); "val_ddad" is the protocol of
# the reference's Trainer.val_ddad (evaluate.evaluate_image_ddad)
EVAL_MODES = {"eigen": 1, "cityscapes": 2, "val_ddad": 3}


@torch.no_grad()
def depth_errors(pred_disp, gt, table, max_region, eval_split="eigen", median_scaling=True, scale=1.0, out=None):
    """pred_disp [B,h,w] fp32 scaled disparity; gt flat fp32 ground truth; table [B,3] int64 (offset, H_gt, W_gt) of the
    batch's images; max_region >= the largest cropped rectangle of the batch (evaluate.region_size).
    eval_split "eigen" / "cityscapes": `Trainer.val`'s protocol with that crop; "val_ddad": mode 3, `Trainer.val_ddad`'s
    (trainer.py:583-623: the DEPTH 1 / disparity is resized, range test 1e-3 < gt < 200, clamp [1e-3, 200], whole map); any
    other name, "ddad" included: `val`'s 80 m range test without a crop.
    -> (errors [B,7] fp64, ratio [B] fp32, count [B] int32); `out`: a contiguous [B,7] fp64 tensor to write the errors to."""
    if pred_disp.dim() != 3:
        raise _abi.PpeaKernelError(f"expected a [B,h,w] disparity batch, got {tuple(pred_disp.shape)}")
    B, h, w = pred_disp.shape
    if table.dim() != 2 or tuple(table.shape) != (B, 3):
        raise _abi.PpeaKernelError(f"ground-truth table {tuple(table.shape)} does not describe a batch of {B} images")
    if gt.dim() != 1:
        raise _abi.PpeaKernelError("the ground truth is one flat buffer")
    dev = pred_disp.device
    p, g, t = ptr(pred_disp, _F32), ptr(gt, _F32), ptr(table, torch.int64)
    errors = torch.empty(B, 7, device=dev, dtype=torch.float64) if out is None else out
    if tuple(errors.shape) != (B, 7):
        raise _abi.PpeaKernelError(f"errors output {tuple(errors.shape)} != {(B, 7)}")
    ratio = torch.empty(B, device=dev, dtype=_F32)
    count = torch.empty(B, device=dev, dtype=torch.int32)
    nbytes = _abi.lib.ppea_depth_errors_workspace_bytes(B, int(max_region))
    if nbytes < 0:
        _abi.check(int(nbytes), "ppea_depth_errors_workspace_bytes")
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    call("ppea_depth_errors_f32", p, g, gt.numel(), t, ptr(ws), ptr(errors, torch.float64), ptr(ratio), ptr(count), B, h, w,
         int(max_region), EVAL_MODES.get(eval_split, 0), int(bool(median_scaling)), float(scale), stream_ptr())
    return errors, ratio, count


@torch.no_grad()
def depth_errors_mean(errors):
    """errors [N,7] fp64 -> their mean over the split [7] fp64, on the device."""
    if errors.dim() != 2 or errors.shape[1] != 7 or errors.shape[0] == 0:
        raise _abi.PpeaKernelError(f"expected [N,7] errors, got {tuple(errors.shape)}")
    mean = torch.empty(7, device=errors.device, dtype=torch.float64)
    call("ppea_depth_errors_mean_f64", ptr(errors, torch.float64), ptr(mean), errors.shape[0], stream_ptr())
    return mean


# ---------------------------------------------------------------------------------------------
# Prediction export: depth at the frame's own size, 16-bit maps, value ranges and colour frames   (csrc/depth_export.hip)
# ---------------------------------------------------------------------------------------------
EXPORT_MODES = {"disp": 0, "depth": 1}      # what is resized: the disparity (val, the benchmark writer) / 1 / disp (val_ddad)
_TARGETS = {}       # (sizes, device) -> the target table on the device; built once, so that a captured call copies nothing
_SCALES = {}        # (value, B, device) -> [B] fp32


def target_sizes(sizes, B):
    """(H, W) or B pairs -> B (H, W) pairs of ints."""
    if len(sizes) == 2 and all(isinstance(v, int) or (torch.is_tensor(v) and v.dim() == 0) for v in sizes):
        sizes = [sizes] * B
    hw = tuple((int(s[0]), int(s[1])) for s in sizes)
    if len(hw) != B:
        raise _abi.PpeaKernelError(f"{len(hw)} target sizes for a batch of {B}")
    if any(h <= 0 or w <= 0 for h, w in hw):
        raise _abi.PpeaKernelError(f"target sizes {hw}")
    return hw


def target_rows(hw):
    """B (H, W) pairs -> ([B] rows (offset, H, W) in pixels, the images back to back; total pixels)."""
    rows, total = [], 0
    for h, w in hw:
        rows.append((total, h, w))
        total += h * w
    return rows, total


def export_targets(sizes, B, device):
    """sizes (H, W) or B pairs -> (table [B,3] int64 on `device` = (offset, H, W) in pixels, the images back to back; the
    dense (H, W) when all sizes are equal, else None; total pixels; largest image).  The device table is kept per size list:
    only the first call with a new list copies anything."""
    hw = target_sizes(sizes, B)
    key = (hw, torch.device(device))
    if key not in _TARGETS:
        rows, total = target_rows(hw)
        _TARGETS[key] = (torch.tensor(rows, dtype=torch.int64).to(key[1]), total, max(h * w for h, w in hw))
    table, total, largest = _TARGETS[key]
    return table, (hw[0] if len(set(hw)) == 1 else None), total, largest


def host_export(images, hw, out=None):
    """What disp_export / colorize return, from B host arrays (the numpy paths of a device="cpu" predictor): the stacked
    tensor when all sizes are equal, else (flat, table)."""
    import numpy as np
    if len(set(hw)) == 1:
        res = torch.from_numpy(np.stack(images))
        return res if out is None else out.view(res.shape).copy_(res)
    flat = torch.from_numpy(np.concatenate([m.reshape((-1,) + m.shape[2:]) for m in images]))
    return (flat if out is None else out.view(flat.shape).copy_(flat)), torch.tensor(target_rows(hw)[0], dtype=torch.int64)


def _planes(x, what):
    if x.dim() == 4 and x.shape[1] == 1:
        x = x[:, 0]
    if x.dim() != 3:
        raise _abi.PpeaKernelError(f"{what}: expected [B,h,w] (or [B,1,h,w]) planes, got {tuple(x.shape)}")
    return x


def _export_out(out, numel, dtype, device, what):
    if out is None:
        return torch.empty(numel, device=device, dtype=dtype)
    if out.dtype != dtype or out.numel() != numel or out.device != device:
        raise _abi.PpeaKernelError(f"{what}: out {out.dtype} {tuple(out.shape)} on {out.device}, expected {numel} values of "
                                   f"{dtype} on {device}")
    return out


@torch.no_grad()
def disp_export(pred, sizes, scale=1.0, lo=1e-3, hi=80.0, mode="disp", dtype=torch.float32, out=None):
    """pred [B,h,w] fp32 scaled disparity -> metric depth at `sizes` ((H, W) or B pairs), cv2.resize(INTER_LINEAR) semantics:
    mode "disp": depth = clamp(scale / resize(pred), lo, hi) (Trainer.val; with scale 5.4, lo 0, hi 80 and (352, 1216) the
    KITTI benchmark writer, eval_depth_ori.py:325-328); mode "depth": clamp(scale * resize(1 / pred), lo, hi) (val_ddad).
    scale: a float, or a [B] fp32 device tensor (`depth_errors`' median ratio, without a copy).  dtype torch.float32: the
    depth; torch.uint16: trunc(depth * 256), the truncation of that same fp32 depth (hi * 256 > 65535 is refused).
    -> [B,H,W] when all sizes are equal, else (flat [sum H W], table [B,3] int64 (offset, H, W)).  out: a contiguous tensor
    of that many values.  One launch; the first call with a new size list also copies its table to the device."""
    pred = _planes(pred, "disp_export")
    B, h, w = pred.shape
    dev = pred.device
    p = ptr(pred, _F32)
    if mode not in EXPORT_MODES:
        raise _abi.PpeaKernelError(f"disp_export: mode {mode!r}, expected one of {sorted(EXPORT_MODES)}")
    if dtype not in (torch.float32, torch.uint16):
        raise _abi.PpeaKernelError(f"disp_export writes float32 or uint16, not {dtype}")
    if torch.is_tensor(scale):
        if tuple(scale.shape) != (B,):
            raise _abi.PpeaKernelError(f"scale {tuple(scale.shape)} for a batch of {B}")
        sc = scale
    else:
        key = (float(scale), B, dev)
        if key not in _SCALES:
            _SCALES[key] = torch.full((B,), float(scale), device=dev, dtype=_F32)
        sc = _SCALES[key]
    table, dense, total, largest = export_targets(sizes, B, dev)
    o = _export_out(out, total, dtype, dev, "disp_export")
    call("ppea_disp_export_f32" if dtype == torch.float32 else "ppea_disp_export_u16", p, ptr(sc, _F32),
         ptr(table, torch.int64), ptr(o, dtype), total, B, h, w, largest, float(lo), float(hi), EXPORT_MODES[mode],
         stream_ptr())
    return o.view(B, *dense) if dense is not None else (o.view(-1), table)


@torch.no_grad()
def plane_range(x, percentile=100.0, out=None):
    """x [B,h,w] fp32 -> [B,2] fp32 (minimum, `percentile`-th percentile) of each plane's values that are not NaN;
    percentile 100: the maximum.  np.percentile's default linear rule on exact order statistics, interpolated in fp64 and
    rounded once; bitwise reproducible.  One launch, no workspace; with `out` nothing is allocated."""
    x = _planes(x, "plane_range")
    B = x.shape[0]
    xp = ptr(x, _F32)
    o = _export_out(out, B * 2, _F32, x.device, "plane_range")
    call("ppea_plane_range_f32", xp, ptr(o, _F32), B, x.shape[1] * x.shape[2], float(percentile), stream_ptr())
    return o.view(B, 2)


@torch.no_grad()
def colorize(x, sizes, rng, lut, out=None):
    """x [B,h,w] fp32 -> RGB uint8 pictures at `sizes` ((H, W) or B pairs): resize (cv2 INTER_LINEAR), (v - vmin) / (vmax -
    vmin) with rng [B,2] fp32 = (vmin, vmax) on the device, and matplotlib's 256-entry lookup in `lut` [256,3] uint8 (vis.lut)
    in one launch.  -> [B,H,W,3] when all sizes are equal, else (flat [sum H W, 3], table).  The bytes of a given `out`
    that belong to no image are left alone; with `out` nothing is allocated."""
    x = _planes(x, "colorize")
    B, h, w = x.shape
    dev = x.device
    xp = ptr(x, _F32)
    if tuple(rng.shape) != (B, 2):
        raise _abi.PpeaKernelError(f"colorize: range {tuple(rng.shape)} for a batch of {B}")
    if tuple(lut.shape) != (256, 3):
        raise _abi.PpeaKernelError(f"colorize: a [256,3] uint8 table, got {tuple(lut.shape)}")
    table, dense, total, largest = export_targets(sizes, B, dev)
    o = _export_out(out, total * 3, torch.uint8, dev, "colorize")
    call("ppea_colorize_u8", xp, ptr(rng, _F32), ptr(lut, torch.uint8), ptr(table, torch.int64), ptr(o, torch.uint8), total, B,
         h, w, largest, stream_ptr())
    return o.view(B, *dense, 3) if dense is not None else (o.view(-1, 3), table)


# ---------------------------------------------------------------------------------------------
# Point clouds: 3D points from a predicted plane, the pose chain of a stream   (csrc/point_cloud.hip)
# ---------------------------------------------------------------------------------------------
_POINT_WS = {}      # (B, largest image, stride, device) -> workspace; built once, so that a captured call allocates nothing
_COLOUR_OFFS = {}   # (sizes, device) -> [B] int64 byte offsets of back-to-back HWC frames


class PointCloud(_NamedTuple):
    """What `point_cloud` fills: xyz [capacity,3] fp32, rgb [capacity,3] uint8 or None, index [capacity] int64 (the flat
    target pixel offset_b + v * W + u), cursor [2] int64 = (points held, points that did not fit), counts [B] int64 = kept
    pixels per image of the last call, fitted or not.  All on the device; nothing of it has been read."""
    xyz: torch.Tensor
    rgb: Optional[torch.Tensor]
    index: torch.Tensor
    cursor: torch.Tensor
    counts: torch.Tensor

    def trim(self):
        """-> (xyz [N,3], rgb [N,3] or None, index [N], dropped): views of the filled part and the number of points that
        did not fit.  Reads `cursor` once (the only copy to the host)."""
        n, dropped = self.cursor.tolist()
        return self.xyz[:n], None if self.rgb is None else self.rgb[:n], self.index[:n], dropped

    def clear(self):
        """Empties the buffers (on the stream: capturable)."""
        self.cursor.zero_()
        return self


def candidate_count(hw, stride):
    """Pixels with u % stride == v % stride == 0 of the (H, W) pairs."""
    return sum(((h - 1) // stride + 1) * ((w - 1) // stride + 1) for h, w in hw)


def new_point_cloud(capacity, B, device, colour=True):
    """An empty `PointCloud` for `capacity` points and calls of B images."""
    return PointCloud(torch.empty(capacity, 3, device=device, dtype=_F32),
                      torch.empty(capacity, 3, device=device, dtype=torch.uint8) if colour else None,
                      torch.empty(capacity, device=device, dtype=torch.int64),
                      torch.zeros(2, device=device, dtype=torch.int64), torch.zeros(B, device=device, dtype=torch.int64))


def _matrices(m, B, what):
    if tuple(m.shape) != (B, 4, 4):
        raise _abi.PpeaKernelError(f"{what} {tuple(m.shape)}, expected {(B, 4, 4)}")
    return ptr(m, _F32)


@torch.no_grad()
def point_cloud(pred, sizes, inv_K, cam_to_world=None, colour=None, colour_off=None, scale=1.0, lo=1e-3, hi=80.0, stride=1,
                edge=0.0, mode="disp", capacity=None, out=None):
    """pred [B,h,w] fp32 scaled disparity -> the 3D points of its depth at `sizes` ((H, W) or B pairs): d = the depth
    `disp_export` computes before its clamp (sizes, scale, mode as there; bit-equal).  Candidates are the pixels with
    u % stride == v % stride == 0; one is kept iff lo < d < hi and (edge <= 0 or |d_n - d| <= edge * d for its 4-neighbours
    in the image).  Point = cam_to_world[b] @ (d * inv_K[b][:3,:3] @ (u, v, 1)), fp32; inv_K [B,4,4] at each image's TARGET
    size, cam_to_world [B,4,4] or None (the camera frame).  colour: uint8 HWC frames at the target sizes in one buffer
    (colour_off [B] int64 device byte offsets; None: back to back) or fp32 [B,3,H,W] in [0,1] (all sizes equal).
    -> `PointCloud`: points in image order, raster order inside an image, deterministic.  capacity: None = the number of
    candidates (nothing can be dropped).  out: a `PointCloud` to append to (its capacity holds).  Three launches, no host
    read; the workspace is kept per (B, largest image, stride, device)."""
    pred = _planes(pred, "point_cloud")
    B, h, w = pred.shape
    dev = pred.device
    p = ptr(pred, _F32)
    if mode not in EXPORT_MODES:
        raise _abi.PpeaKernelError(f"point_cloud: mode {mode!r}, expected one of {sorted(EXPORT_MODES)}")
    stride = int(stride)
    if stride < 1:
        raise _abi.PpeaKernelError(f"point_cloud: stride {stride}")
    if torch.is_tensor(scale):
        if tuple(scale.shape) != (B,):
            raise _abi.PpeaKernelError(f"scale {tuple(scale.shape)} for a batch of {B}")
        sc = scale
    else:
        key = (float(scale), B, dev)
        if key not in _SCALES:
            _SCALES[key] = torch.full((B,), float(scale), device=dev, dtype=_F32)
        sc = _SCALES[key]
    table, dense, total, largest = export_targets(sizes, B, dev)
    hw = target_sizes(sizes, B)
    kp = _matrices(inv_K, B, "inv_K")
    mp = None if cam_to_world is None else _matrices(cam_to_world, B, "cam_to_world")
    cmode, cp, op = 0, None, None
    if colour is not None:
        if colour.dtype == torch.uint8:
            cmode = 1
            if colour_off is None:
                if colour.numel() != total * 3:
                    raise _abi.PpeaKernelError(f"colour: {colour.numel()} bytes for {total} pixels")
                key = (hw, dev)
                if key not in _COLOUR_OFFS:
                    _COLOUR_OFFS[key] = (table[:, 0] * 3).contiguous()
                colour_off = _COLOUR_OFFS[key]
            elif tuple(colour_off.shape) != (B,):
                raise _abi.PpeaKernelError(f"colour_off {tuple(colour_off.shape)} for a batch of {B}")
            cp, op = ptr(colour, torch.uint8), ptr(colour_off, torch.int64)
        elif colour.dtype == _F32:
            cmode = 2
            if dense is None or tuple(colour.shape) != (B, 3, *dense):
                raise _abi.PpeaKernelError(f"fp32 colour {tuple(colour.shape)} needs every target equal to its (H, W); "
                                           f"targets {hw}")
            cp = ptr(colour, _F32)
        else:
            raise _abi.PpeaKernelError(f"colour {colour.dtype}: uint8 HWC frames or fp32 [B,3,H,W]")
    if out is None:
        cap = candidate_count(hw, stride) if capacity is None else int(capacity)
        if cap < 0:
            raise _abi.PpeaKernelError(f"point_cloud: capacity {cap}")
        out = new_point_cloud(cap, B, dev, cmode != 0)
    else:
        cap = out.xyz.shape[0]
        if capacity is not None and int(capacity) != cap:
            raise _abi.PpeaKernelError(f"point_cloud: capacity {capacity}, out holds {cap}")
        if tuple(out.xyz.shape) != (cap, 3) or tuple(out.index.shape) != (cap,) or tuple(out.cursor.shape) != (2,) \
                or tuple(out.counts.shape) != (B,) or (cmode != 0 and (out.rgb is None or tuple(out.rgb.shape) != (cap, 3))):
            raise _abi.PpeaKernelError(f"point_cloud: out does not fit {cap} points of {B} images"
                                       f"{' with colour' if cmode else ''}")
    key = (B, largest, stride, dev)
    if key not in _POINT_WS:
        nbytes = _abi.lib.ppea_point_cloud_workspace_bytes(B, largest, stride)
        if nbytes < 0:
            _abi.check(int(nbytes), "ppea_point_cloud_workspace_bytes")
        _POINT_WS[key] = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    call("ppea_point_cloud_f32", p, ptr(sc, _F32), ptr(table, torch.int64), B, h, w, largest, float(lo), float(hi),
         EXPORT_MODES[mode], stride, float(edge), kp, mp, cp, op, cmode, ptr(out.xyz, _F32),
         ptr(out.rgb, torch.uint8) if cmode else None, ptr(out.index, torch.int64), cap, ptr(out.cursor, torch.int64),
         ptr(out.counts, torch.int64), ptr(_POINT_WS[key], torch.uint8), stream_ptr())
    return out


@torch.no_grad()
def pose_accumulate(world, pose, present):
    """world [B,4,4] fp32, in place: world[b] @ pose[b,0] where present[b,0], the identity elsewhere.  pose [B,F,4,4] and
    present [B,F] bool are a stream push's; pose[b,0] maps frame t to frame t-1, so `world` stays the camera-to-world matrix
    of the newest frame, the clip's first frame being the world.  A plain fp32 product chain (fixed summation order, no
    re-orthonormalisation).  One launch."""
    B = world.shape[0]
    if tuple(world.shape) != (B, 4, 4) or pose.dim() != 4 or tuple(pose.shape) != (B, pose.shape[1], 4, 4) \
            or pose.shape[1] < 1 or tuple(present.shape) != tuple(pose.shape[:2]):
        raise _abi.PpeaKernelError(f"pose_accumulate: world {tuple(world.shape)}, pose {tuple(pose.shape)}, present "
                                   f"{tuple(present.shape)}")
    if present.dtype == torch.bool:
        present = present.view(torch.uint8)
    call("ppea_pose_accumulate_f32", ptr(world, _F32), ptr(pose, _F32), ptr(present, torch.uint8), B, pose.shape[1],
         stream_ptr())
    return world


# ---------------------------------------------------------------------------------------------
# KITTI ground truth from raw LiDAR: kitti_utils.generate_depth_map for a ragged batch of scans   (csrc/kitti_gt.hip)
# ---------------------------------------------------------------------------------------------
def _host_i64(t, what):
    """Address of a host array the launcher reads itself (grid sizes, refusals): a contiguous int64 CPU tensor."""
    if not torch.is_tensor(t) or t.is_cuda or t.dtype != torch.int64 or not t.is_contiguous():
        raise _abi.PpeaKernelError(f"{what}: a contiguous int64 tensor on the host")
    return _ct.c_void_p(t.data_ptr())


@torch.no_grad()
def velodyne_depth_maps(points, point_offsets, P, table, vel_depth=True):
    """points [sum N,4] fp32 (device): B velodyne scans one after another (column 3 is ignored); point_offsets [B+1] int64 on
    the HOST; P [B,3,4] fp64 (device): each scan's velodyne -> image matrix; table [B,3] int64 on the HOST: (offset, H, W) of
    each map in the result -- the values of `DeviceGroundTruth.table`.  vel_depth: the depth is the point's own x
    (export_gt_depth.py), else the projected q2.
    -> flat fp32 [max(offset + H * W)] on the device: the sparse depth maps of kitti_utils.generate_depth_map (last point per
    pixel, minimum per duplicated sub2ind key at its first point's pixel, negatives to 0), every pixel written."""
    if points.dim() != 2 or points.shape[1] != 4:
        raise _abi.PpeaKernelError(f"expected [N,4] velodyne points, got {tuple(points.shape)}")
    if P.dim() != 3 or tuple(P.shape[1:]) != (3, 4):
        raise _abi.PpeaKernelError(f"expected [B,3,4] projection matrices, got {tuple(P.shape)}")
    B = P.shape[0]
    if tuple(table.shape) != (B, 3) or tuple(point_offsets.shape) != (B + 1,):
        raise _abi.PpeaKernelError(f"table {tuple(table.shape)} / point offsets {tuple(point_offsets.shape)} do not describe "
                                   f"{B} scans")
    po, tb = _host_i64(point_offsets, "point_offsets"), _host_i64(table, "table")
    if P.device != points.device:
        raise _abi.PpeaKernelError("points and P live on different devices")
    pp, pm = ptr(points, _F32), ptr(P, torch.float64)
    # what the launcher cannot see: the buffers' lengths.  (Its own refusals -- B <= 0, descending offsets, negative sizes --
    # come back as PPEA_ERR_ARG before anything is launched.)
    if B and int(point_offsets.max()) > points.shape[0]:
        raise _abi.PpeaKernelError(f"point offsets reach {int(point_offsets.max())}, the buffer holds {points.shape[0]} points")
    sizes = table[:, 1] * table[:, 2]
    pixels = int(sizes.clamp(min=0).sum()) if B else 0
    length = int((table[:, 0] + sizes).max()) if B else 0
    nbytes = _abi.lib.ppea_velodyne_depth_workspace_bytes(pixels)
    if nbytes < 0:
        _abi.check(int(nbytes), "ppea_velodyne_depth_workspace_bytes")
    out = torch.empty(max(length, 0), device=points.device, dtype=_F32)
    ws = torch.empty(nbytes, device=points.device, dtype=torch.uint8)
    call("ppea_velodyne_depth_f32", pp, po, B, pm, tb, int(bool(vel_depth)), ptr(out), ptr(ws), stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------
# Input pipeline on uint8 frames: Pillow's LANCZOS resize and the PIL-path ColorJitter   (csrc/input_pipeline.hip)
# ---------------------------------------------------------------------------------------------
JITTER_PARAM_WORDS = 10


def _taps(table, outsize, what):
    if table.dim() != 2 or table.shape[0] != outsize or table.shape[1] < 3:
        raise _abi.PpeaKernelError(f"{what} tap table {tuple(table.shape)} does not describe {outsize} outputs")
    return ptr(table, torch.int32), table.shape[1] - 2


def _lanczos_resize(srcs, dims, out_hw, taps_h, taps_v, flip, nonzero, horizontal):
    """The body of `lanczos_resize_u8` and `lanczos_resize_view_u8`: the checks they share, the horizontal pass over srcs
    (each `dims` = (n, C, Hin, Win); `horizontal(ptrs, taps, kmax, *rest)` calls the entry point of their layout; skipped
    when taps_h is None) and the vertical pass."""
    n, C, Hin, Win = dims
    N, (Hout, Wout) = n * len(srcs), out_hw
    for s in srcs:
        if not s.is_cuda:
            raise _abi.PpeaKernelError("PPEA-Depth HIP kernels need tensors on a HIP device (no CPU fallback); got a CPU tensor")
        if s.dtype != torch.uint8:
            raise _abi.PpeaKernelError(f"expected torch.uint8, got {s.dtype}")
    if taps_v is None and Hin != Hout:
        raise _abi.PpeaKernelError("a change of height needs the vertical pass")
    for t in (flip, nonzero):
        if t is not None and tuple(t.shape) != (N,):
            raise _abi.PpeaKernelError(f"expected one flag per image ({N}), got {tuple(t.shape)}")
    cur = srcs[0]
    if taps_h is not None:
        tp, kmax = _taps(taps_h, Wout, "horizontal")
        ptrs = (_ct.c_void_p * len(srcs))(*[s.data_ptr() for s in srcs])
        cur = torch.empty(N, C, Hin, Wout, device=cur.device, dtype=torch.uint8)
        horizontal(ptrs, tp, kmax, ptr(flip, torch.int32), ptr(nonzero, torch.int32), ptr(cur), Hin, Win, Wout, stream_ptr())
    if taps_v is not None:
        tp, kmax = _taps(taps_v, Hout, "vertical")
        out = torch.empty(N, C, Hout, Wout, device=cur.device, dtype=torch.uint8)
        call("ppea_lanczos_v_u8", ptr(cur, torch.uint8), tp, kmax, ptr(out), N * C, Hin, Hout, Wout, stream_ptr())
        cur = out
    return cur


@torch.no_grad()
def lanczos_resize_u8(src, out_hw, taps_h=None, taps_v=None, flip=None, nonzero=None):
    """src: uint8 [N,C,Hin,Win], or a list of such tensors of one shape (read as if concatenated along N, without the
    copy) -> uint8 [N,C,Hout,Wout].  taps_h [Wout, 2+k] / taps_v [Hout, 2+k] int32 (input_pipeline.compact_taps); None
    skips that pass (its input and output sizes are then equal).  Horizontal pass first, 8-bit intermediate.
    flip [N] int32: non-zero = image n is mirrored left-right first (needs taps_h); nonzero [N] int32: written,
    1 where image n holds a non-zero byte (needs taps_h)."""
    srcs = list(src) if isinstance(src, (list, tuple)) else [src]
    if not srcs or any(s.dim() != 4 or s.shape != srcs[0].shape for s in srcs):
        raise _abi.PpeaKernelError("expected uint8 [N,C,H,W] images of one shape")
    if not all(s.is_contiguous() for s in srcs):
        raise _abi.PpeaKernelError("non-contiguous tensor passed to a HIP kernel")
    n, C, Hin, Win = srcs[0].shape
    if taps_h is None and (Win != out_hw[1] or flip is not None or nonzero is not None):
        raise _abi.PpeaKernelError("the flip, the non-zero mark and a change of width need the horizontal pass")
    if taps_h is None and len(srcs) != 1:
        raise _abi.PpeaKernelError("several sources are read by the horizontal pass only")
    return _lanczos_resize(srcs, (n, C, Hin, Win), out_hw, taps_h, taps_v, flip, nonzero,
                           lambda ptrs, tp, kmax, fl, nz, *rest: call("ppea_lanczos_h_u8", ptrs, len(srcs), n * C, tp, kmax, fl,
                                                                     C, nz, *rest))


@torch.no_grad()
def lanczos_resize_view_u8(src, out_hw, taps_h, taps_v=None, flip=None, nonzero=None):
    """`lanczos_resize_u8` over VIEWS: src is a uint8 [n,Hin,Win,C] tensor as a decoder returns it (HWC), or any view of
    that shape (a window of a wider image, the top rows of a taller one, `planar.permute(0, 2, 3, 1)`), or a list of such
    views of one shape and one set of strides (read as if concatenated along n) -> uint8 [N,C,Hout,Wout], planar.  Nothing
    is copied: the horizontal pass reads the views through their strides, so taps_h is always given
    (input_pipeline.identity_taps when the width stays).  taps_v / flip / nonzero as in `lanczos_resize_u8`."""
    srcs = list(src) if isinstance(src, (list, tuple)) else [src]
    if not srcs or any(s.dim() != 4 or s.shape != srcs[0].shape or s.stride() != srcs[0].stride() for s in srcs):
        raise _abi.PpeaKernelError("expected uint8 [n,H,W,C] views of one shape and one set of strides")
    if taps_h is None:
        raise _abi.PpeaKernelError("a view is read by the horizontal pass: give its tap table")
    n, Hin, Win, C = srcs[0].shape
    item, row, pixel, channel = srcs[0].stride()              # uint8: elements are bytes
    return _lanczos_resize(srcs, (n, C, Hin, Win), out_hw, taps_h, taps_v, flip, nonzero,
                           lambda ptrs, tp, kmax, *rest: call("ppea_lanczos_h_view_u8", ptrs, len(srcs), n, C, pixel, row,
                                                              channel, item, tp, kmax, *rest))


def ragged_row_prefix(desc):
    """Host int32 [N,4] descriptor (byte offset, H, W, size class) -> int32 [N+1]: the rows of the images before n."""
    prefix = torch.zeros(desc.shape[0] + 1, dtype=torch.int64)
    prefix[1:] = desc[:, 1].to(torch.int64).cumsum(0)
    return prefix.to(torch.int32)


def _class_taps(table, outsize, what):
    if table.dim() != 3 or table.shape[0] < 1 or table.shape[1] != outsize or table.shape[2] < 3:
        raise _abi.PpeaKernelError(f"{what} class tap table {tuple(table.shape)} does not describe {outsize} outputs per class")
    return ptr(table, torch.int32), table.shape[0], table.shape[2] - 2


@torch.no_grad()
def lanczos_resize_ragged_u8(buf, desc, out_hw, taps_h, taps_v, flip=None, nonzero=None, scratch=None):
    """`lanczos_resize_view_u8` for N interleaved-RGB (HWC) frames of DIFFERENT sizes in one launch pair -> uint8
    [N,3,Hout,Wout].  buf: 1-D uint8 device buffer, the frames back to back, fewer than 2^31 bytes.  desc: HOST int32 [N,4]
    = (byte offset, H, W, size class), H = W = 0 an absent frame (written as zeros, its `nonzero` 0); or the pair (that host
    tensor, its device copy: int32 [N * 4 + N + 1], the descriptor followed by `ragged_row_prefix`), as a caller has it that
    uploads the words with its other parameters -- otherwise they are uploaded here.  The host descriptor is checked before
    anything is launched.  taps_h [K,Wout,2+k] / taps_v [K,Hout,2+k] int32 device tables of the K size classes
    (input_pipeline.compact_taps rows, zero-padded to the longest; identity_taps where a size stays).  flip / nonzero [N]
    as in `lanczos_resize_u8`.  scratch: uint8 device tensor of at least N * 3 * max(H) * Wout elements to hold the 8-bit
    intermediate (rows at or beyond an image's H are neither written nor read); default: allocated here."""
    host, words = desc if isinstance(desc, (list, tuple)) else (desc, None)
    if host.is_cuda or host.dtype != torch.int32 or host.dim() != 2 or host.shape[1] != 4 or host.shape[0] < 1:
        raise _abi.PpeaKernelError("expected the descriptor as a host int32 [N,4] tensor (byte offset, H, W, size class)")
    host = host.contiguous()
    N, (Hout, Wout) = host.shape[0], out_hw
    bp = ptr(buf, torch.uint8)
    if buf.dim() != 1 or buf.numel() < 1:
        raise _abi.PpeaKernelError(f"expected a 1-D byte buffer, got {tuple(buf.shape)}")
    if buf.numel() >= 1 << 31:
        raise _abi.PpeaKernelError(f"{buf.numel()} bytes of frames: the descriptor's offsets are 32 bits")
    for t in (flip, nonzero):
        if t is not None and tuple(t.shape) != (N,):
            raise _abi.PpeaKernelError(f"expected one flag per image ({N}), got {tuple(t.shape)}")
    th, K, kh = _class_taps(taps_h, Wout, "horizontal")
    tv, Kv, kv = _class_taps(taps_v, Hout, "vertical")
    if K != Kv:
        raise _abi.PpeaKernelError(f"{K} horizontal and {Kv} vertical size classes")
    off, H, W, cls = (host[:, i].to(torch.int64) for i in range(4))
    if bool(((off < 0) | (H < 0) | (W < 0) | ((H == 0) != (W == 0))).any()):
        raise _abi.PpeaKernelError("descriptor: negative entry, or only one of H and W zero")
    if bool(((cls < 0) | (cls >= K)).any()):
        raise _abi.PpeaKernelError(f"descriptor: size class outside the {K} classes of the tap tables")
    if bool((off + H * W * 3 > buf.numel()).any()):
        raise _abi.PpeaKernelError(f"descriptor: a frame reaches past the buffer's {buf.numel()} bytes")
    Hcap = max(int(H.max()), 1)
    if words is None:
        words = torch.cat([host.reshape(-1), ragged_row_prefix(host)]).to(buf.device)
    if tuple(words.shape) != (N * 5 + 1,):
        raise _abi.PpeaKernelError(f"device descriptor {tuple(words.shape)}: expected {N * 5 + 1} words (descriptor, row prefix)")
    dp = ptr(words, torch.int32)
    pp = _ct.c_void_p(words.data_ptr() + N * 16)
    hp = _ct.c_void_p(host.data_ptr())
    if scratch is None:
        scratch = torch.empty(N * 3 * Hcap * Wout, device=buf.device, dtype=torch.uint8)
    elif scratch.device != buf.device or scratch.numel() < N * 3 * Hcap * Wout:
        raise _abi.PpeaKernelError(f"scratch holds {scratch.numel()} bytes on {scratch.device}, the intermediate needs "
                                   f"{N * 3 * Hcap * Wout} on {buf.device}")
    sp = ptr(scratch, torch.uint8)
    out = torch.empty(N, 3, Hout, Wout, device=buf.device, dtype=torch.uint8)
    call("ppea_lanczos_h_ragged_u8", bp, buf.numel(), hp, dp, pp, N, th, K, kh, ptr(flip, torch.int32),
         ptr(nonzero, torch.int32), sp, Hcap, Wout, stream_ptr())
    call("ppea_lanczos_v_ragged_u8", sp, hp, dp, N, tv, K, kv, ptr(out), Hcap, Hout, Wout, stream_ptr())
    return out


@torch.no_grad()
def color_jitter_u8(img, params, nonzero=None):
    """img uint8 [N,3,H,W]; params int32 [N,10] (input_pipeline.pack_jitter_params); nonzero [N] int32 or None (0 = the
    image is blank and is never jittered) -> (color, color_aug) fp32 [N,3,H,W] = img / 255, jitter(img) / 255."""
    if img.dim() != 4 or img.shape[1] != 3:
        raise _abi.PpeaKernelError(f"expected uint8 [N,3,H,W], got {tuple(img.shape)}")
    N, _, H, W = img.shape
    if tuple(params.shape) != (N, JITTER_PARAM_WORDS) or (nonzero is not None and tuple(nonzero.shape) != (N,)):
        raise _abi.PpeaKernelError(f"parameter table {tuple(params.shape)} does not describe {N} images")
    im, pp, nz = ptr(img, torch.uint8), ptr(params, torch.int32), ptr(nonzero, torch.int32)
    nbytes = _abi.lib.ppea_color_jitter_workspace_bytes(N, H, W)
    if nbytes < 0:
        _abi.check(int(nbytes), "ppea_color_jitter_workspace_bytes")
    ws = torch.empty(nbytes, device=img.device, dtype=torch.uint8)
    color = torch.empty(N, 3, H, W, device=img.device, dtype=_F32)
    aug = torch.empty_like(color)
    call("ppea_color_jitter_u8", im, pp, nz, ptr(ws), ptr(color), ptr(aug), N, H, W, stream_ptr())
    return color, aug


@torch.no_grad()
def repeat_rows(src, reps):
    """src fp32 [R, ...] -> [R, reps, ...]: every row repeated `reps` times, one launch."""
    out = torch.empty((src.shape[0], reps) + tuple(src.shape[1:]), device=src.device, dtype=_F32)
    call("ppea_repeat_rows_f32", ptr(src, _F32), ptr(out), src.shape[0], reps, src[0].numel(), stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------
# A2 + block glue: y = act(BN_a(z1) [+ BN_b(z2)]) [* mask[n]] [+ r1] [+ s * r2]   (csrc/bn_fused.hip)
# ---------------------------------------------------------------------------------------------
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2


def _ptr_array(ts):
    """host array of device pointers (NULL for an absent tensor, e.g. the second branch's)."""
    arr = (_ct.c_void_p * len(ts))()
    for i, t in enumerate(ts):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def _bn_operands(z1, others, params, mask):
    """Operand prologue of the fused BatchNorm Functions: z1 contiguous; the other activations (second branch, residuals)
    contiguous in z1's dtype; gamma / beta detached, contiguous fp32; the per-sample mask flat fp32.
    -> (z1, others, params, mask, (N, C, HW)), absent operands staying None."""
    z1 = z1.contiguous()
    others = [None if t is None else t.contiguous().to(z1.dtype) for t in others]
    params = [None if p is None else p.detach().float().contiguous() for p in params]
    maskf = None if mask is None else mask.detach().reshape(-1).float().contiguous()
    N, C = z1.shape[0], z1.shape[1]
    return z1, others, params, maskf, (N, C, z1.numel() // (N * C))


def _bn_bwd_sums(dy, z1, z2, stats, maskf, act, dyb=None):
    """Per-channel sums of a BatchNorm backward, [3][C] = sum dy' | sum dy' xhat1 | sum dy' xhat2 (dy' = dy through the
    activation and the mask): one launch where a workgroup can finish a channel, per-plane partials + finalize for large
    planes.  `dyb`: a second gradient of the same output, merged in the one-launch kernel (round(dy + dyb), stored for the
    apply launch), by an element-wise add in front of the two-launch form.  -> (sums, the merged dy, one launch served)."""
    N, C = z1.shape[0], z1.shape[1]
    HW = z1.numel() // (N * C)
    sfx = _suffix(z1)
    sums = torch.empty(3, C, device=z1.device, dtype=_F32)
    if dyb is not None:
        dyb = dyb.contiguous().to(z1.dtype)
        dym = torch.empty_like(z1)
        final = try_call(f"ppea_bn_bwd_reduce_final_dup_{sfx}", ptr(dy), ptr(dyb), ptr(dym), ptr(z1), ptr(z2), stats,
                         ptr(maskf), ptr(sums), act, N, C, HW, stream_ptr())
        dy = dym if final else dy + dyb
    else:
        final = try_call(f"ppea_bn_bwd_reduce_final_{sfx}", ptr(dy), ptr(z1), ptr(z2), stats, ptr(maskf), ptr(sums), act,
                         N, C, HW, stream_ptr())
    if not final:                           # large planes: per-plane partials + finalize
        partial = torch.empty(C * N * 3, device=z1.device, dtype=_F32)
        call(f"ppea_bn_bwd_reduce_{sfx}", ptr(dy), ptr(z1), ptr(z2), stats, ptr(maskf), ptr(partial), act, N, C, HW,
             stream_ptr())
        call("ppea_bn_bwd_finalize_f32", ptr(partial), N, C, ptr(sums), stream_ptr())
    return sums, dy, final


def _bn_grads(ctx, sums, two, dy):
    """Gradient epilogue of the two-branch Functions: (d gamma1, d beta1, d gamma2, d beta2) from `sums` = d beta | d gamma1 |
    d gamma2 in the parameters' dtypes, and (d r1, d r2) from the output gradient."""
    n = ctx.needs_input_grad
    dg1 = sums[1].to(ctx.pdt[0]) if n[1] else None
    db1 = sums[0].to(ctx.pdt[1]) if n[2] else None
    dg2 = sums[2].to(ctx.pdt[2]) if (two and n[6]) else None
    db2 = sums[0].to(ctx.pdt[2]) if (two and n[7]) else None
    dr1 = dy if ctx.has[0] else None
    dr2 = (dy if ctx.r2_scale == 1.0 else dy * ctx.r2_scale) if ctx.has[1] else None
    return dg1, db1, dg2, db2, dr1, dr2


def bn_batch_stats(z, eps, momentum, running_mean=None, running_var=None):
    """(mean, biased var, invstd) of z over (N,H,W); optionally updates running stats in the same launch."""
    z = z.contiguous()
    N, C = z.shape[0], z.shape[1]
    HW = z.numel() // (N * C)
    dev = z.device
    out = torch.empty(3, C, device=dev, dtype=_F32)
    if try_call(f"ppea_bn_stats_final_{_suffix(z)}", ptr(z), N, C, HW, float(eps), float(momentum), ptr(out[0]), ptr(out[1]),
                ptr(out[2]), ptr(running_mean), ptr(running_var), stream_ptr()):
        return out[0], out[1], out[2]       # small channels: statistics final in one launch
    partial = torch.empty(C * N * 2, device=dev, dtype=_F32)
    call(f"ppea_bn_stats_{_suffix(z)}", ptr(z), ptr(partial), N, C, HW, stream_ptr())
    call("ppea_bn_finalize_f32", ptr(partial), N, C, HW, float(eps), float(momentum), ptr(out[0]), ptr(out[1]),
         ptr(out[2]), ptr(running_mean), ptr(running_var), stream_ptr())
    return out[0], out[1], out[2]


def bn_batch_stats_from_sums(sums, count, eps, momentum, running_mean=None, running_var=None):
    """(mean, biased var, invstd) from the producing GEMM's partial sums [C, P, 2] (pwconv_frozen(..., want_sums=True)):
    one small launch instead of a statistics pass over the activation; updates the running statistics."""
    C, P = sums.shape[0], sums.shape[1]
    out = torch.empty(3, C, device=sums.device, dtype=_F32)
    call("ppea_bn_finalize_sums_f32", ptr(sums, _F32), P, C, int(count), float(eps), float(momentum), ptr(out[0]), ptr(out[1]),
         ptr(out[2]), ptr(running_mean), ptr(running_var), stream_ptr())
    return out[0], out[1], out[2]


def bn_local_stats_packed(z):
    """SyncBN wire format of the local statistics: [mean(C) | biased var(C) | count] fp32."""
    z = z.contiguous()
    N, C = z.shape[0], z.shape[1]
    HW = z.numel() // (N * C)
    packed = torch.empty(2 * C + 1, device=z.device, dtype=_F32)
    if try_call(f"ppea_bn_stats_packed_{_suffix(z)}", ptr(z), N, C, HW, ptr(packed), stream_ptr()):
        return packed
    partial = torch.empty(C * N * 2, device=z.device, dtype=_F32)
    call(f"ppea_bn_stats_{_suffix(z)}", ptr(z), ptr(partial), N, C, HW, stream_ptr())
    call("ppea_bn_finalize_packed_f32", ptr(partial), N, C, HW, ptr(packed), stream_ptr())
    return packed


def bn_sync_combine(gathered, eps, momentum, running_mean=None, running_var=None):
    """gathered [world, 2C+1] -> (mean, invstd) of the global batch; running statistics updated in the launch."""
    world, C = gathered.shape[0], (gathered.shape[1] - 1) // 2
    out = torch.empty(2, C, device=gathered.device, dtype=_F32)
    call("ppea_bn_sync_combine_f32", ptr(gathered, _F32), world, C, float(eps), float(momentum), ptr(out[0]),
         ptr(out[1]), ptr(running_mean), ptr(running_var), stream_ptr())
    return out[0], out[1]


class _BnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z1, g1, b1, mean1, invstd1, z2, g2, b2, mean2, invstd2, mask, r1, r2, r2_scale, act,
                count, group):
        z1, (z2, r1, r2), (g1f, b1f, g2f, b2f), maskf, (N, C, HW) = _bn_operands(z1, (z2, r1, r2), (g1, b1, g2, b2), mask)
        y = torch.empty_like(z1)
        st = (mean1, invstd1, g1f, b1f, mean2, invstd2, g2f, b2f)
        call(f"ppea_bn_apply_{_suffix(z1)}", ptr(z1), ptr(z2), _ptr_array(st), ptr(maskf), ptr(r1), ptr(r2),
             float(r2_scale), ptr(y), int(act), N, C, HW, stream_ptr())
        ctx.save_for_backward(z1, z2, mean1, invstd1, g1f, b1f, mean2, invstd2, g2f, b2f, maskf)
        ctx.act, ctx.r2_scale, ctx.count, ctx.group = int(act), float(r2_scale), float(count), group
        ctx.has = (r1 is not None, r2 is not None)
        ctx.pdt = (g1.dtype, b1.dtype, None if g2 is None else g2.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        z1, z2, mean1, invstd1, g1f, b1f, mean2, invstd2, g2f, b2f, maskf = ctx.saved_tensors
        N, C = z1.shape[0], z1.shape[1]
        HW = z1.numel() // (N * C)
        dy = dy.contiguous().to(z1.dtype)
        st = _ptr_array((mean1, invstd1, g1f, b1f, mean2, invstd2, g2f, b2f))
        sums, _, _ = _bn_bwd_sums(dy, z1, z2, st, maskf, ctx.act)
        inv_count = 1.0 / ctx.count
        gscale = None
        if ctx.group is not None:                      # SyncBN: sums of the global batch (ctx.count is the global count)
            reduce_sums(sums, ctx.group[0])
            gscale = 1.0 / sync_world(ctx.group[0])    # d gamma / d beta: see _SyncBnAct
        dz1 = torch.empty_like(z1)
        dz2 = None if z2 is None else torch.empty_like(z2)
        call(f"ppea_bn_bwd_apply_{_suffix(z1)}", ptr(dy), ptr(z1), ptr(z2), st, ptr(maskf), ptr(sums), inv_count,
             ptr(dz1), ptr(dz2), ctx.act, N, C, HW, stream_ptr())
        if gscale is not None:
            sums = sums * gscale
        dg1, db1, dg2, db2, dr1, dr2 = _bn_grads(ctx, sums, z2 is not None, dy)
        return (dz1, dg1, db1, None, None, dz2, dg2, db2, None, None, None, dr1, dr2, None, None, None, None)


BN_CHANNEL = True          # small channels: statistics + apply (and reduce + apply) as ONE launch each


def bn_channel_ok(z):
    """Whole channel in one workgroup's registers: csrc/bn_fused.hip bn_fwd_channel / bn_bwd_channel."""
    if not (BN_CHANNEL and z.is_cuda and z.dim() == 4 and z.dtype in (_F32, _BF16)):
        return False
    N, C = z.shape[0], z.shape[1]
    HW = z.shape[2] * z.shape[3]
    return C >= 64 and HW % 8 == 0 and N * HW <= 16384


def _other_stream_grad(g):
    """A gradient that may have been produced on ANOTHER stream (the second consumer of a BatchNorm output is the block's
    adapter, which runs on a forked side stream) and is read by a kernel launched here: mark it as in use by the current
    stream.  The autograd engine makes the consumer stream wait for the producer, but for a gradient that is not accumulated
    with another one it does not record the consumer on the tensor -- the block would go back to the producer stream's pool
    as soon as this backward returns and could be rewritten by that stream's next allocation while the kernel launched here
    has not run yet.  (A precaution: the alias is only handed to consumers on the SAME stream, see rka.ConvFFN.forward.)"""
    if g is not None and g.is_cuda:
        g.record_stream(torch.cuda.current_stream())


class _BnActChannel(torch.autograd.Function):
    """y = act(BN1(z1) [+ BN2(z2)]) [* mask[n]] [+ r1] [+ s * r2] with batch statistics, running-statistics update and
    the saved (mean, invstd) in ONE launch; backward (sums + dz) in one launch."""

    @staticmethod
    def forward(ctx, z1, g1, b1, rm1, rv1, z2, g2, b2, rm2, rv2, mask, r1, r2, r2_scale, act, eps, momentum, skip=False,
                dup=False, sums=None):
        z1_in = z1
        z1, (z2, r1, r2), (g1f, b1f, g2f, b2f), maskf, (N, C, HW) = _bn_operands(z1, (z2, r1, r2), (g1, b1, g2, b2), mask)
        st = torch.empty(4, C, device=z1.device, dtype=_F32)          # mean1 | invstd1 | mean2 | invstd2
        y = torch.empty_like(z1)
        if sums is not None and z2 is None:
            # statistics from the producing GEMM's epilogue: [C][P][2] partial (sum, sum of squares) of the stored values
            sums = sums.contiguous()
            call(f"ppea_bn_fwd_channel_sums_{_suffix(z1)}", ptr(z1), ptr(sums, _F32), int(sums.shape[1]), _ptr_array((g1f, b1f)),
                 _ptr_array((rm1, rv1, st[0], st[1])), float(eps), float(momentum), ptr(maskf), ptr(r1), ptr(r2),
                 float(r2_scale), ptr(y), int(act), N, C, HW, stream_ptr())
        else:
            call(f"ppea_bn_fwd_channel_{_suffix(z1)}", ptr(z1), ptr(z2), _ptr_array((g1f, b1f, g2f, b2f)),
                 _ptr_array((rm1, rv1, rm2, rv2, st[0], st[1], st[2], st[3])), float(eps), float(momentum), ptr(maskf),
                 ptr(r1), ptr(r2), float(r2_scale), ptr(y), int(act), N, C, HW, stream_ptr())
        ctx.save_for_backward(z1, z2, st, g1f, b1f, g2f, b2f, maskf)
        ctx.act, ctx.r2_scale = int(act), float(r2_scale)
        ctx.has = (r1 is not None, r2 is not None)
        ctx.pdt = (g1.dtype, b1.dtype, None if g2 is None else g2.dtype)
        ctx.mark_non_differentiable(st)
        ctx.set_materialize_grads(False)         # no zero-filled "gradient" of the statistics output per backward call
        ctx.skip, ctx.dup = bool(skip), bool(dup)
        outs = (y, st)
        if skip:
            # third output: z1 itself, for the block's residual use -- its gradient comes back HERE and is added in the
            # backward launch (autograd would otherwise add the two gradients of z1 with one more element-wise kernel)
            outs += (z1_in,)
        if dup:
            # last output: y once more (same storage) for its SECOND consumer (a block's adapter next to its first 1x1
            # conv): the two gradients arrive separately and are added in the backward launch
            outs += (y.detach(),)
        return outs

    @staticmethod
    def backward(ctx, dy, _dst, *rest):
        rest = list(rest)
        dskip = rest.pop(0) if ctx.skip else None
        dyb = rest.pop(0) if ctx.dup else None
        z1, z2, st, g1f, b1f, g2f, b2f, maskf = ctx.saved_tensors
        N, C = z1.shape[0], z1.shape[1]
        HW = z1.numel() // (N * C)
        _other_stream_grad(dyb)
        if dy is None:
            dy, dyb = (dyb, None) if dyb is not None else (torch.zeros_like(z1), None)
        dy = dy.contiguous().to(z1.dtype)
        if dyb is not None:
            dyb = dyb.contiguous().to(z1.dtype)
        sums = torch.empty(3, C, device=z1.device, dtype=_F32)
        dz1 = torch.empty_like(z1)
        dz2 = None if z2 is None else torch.empty_like(z2)
        stats = _ptr_array((st[0], st[1], g1f, b1f, st[2] if z2 is not None else None,
                              st[3] if z2 is not None else None, g2f, b2f))
        if dskip is not None:
            dskip = dskip.contiguous().to(z1.dtype)
        if dyb is not None:
            if ctx.has[0] or ctx.has[1]:
                dy = dy + dyb                                # (r1 / r2 receive dy itself: not a block's first BatchNorm)
                dyb = None
        if dyb is not None:
            call(f"ppea_bn_bwd_channel_dup_{_suffix(z1)}", ptr(dy), ptr(dyb), ptr(z1), ptr(z2), stats, ptr(maskf),
                 1.0 / float(N * HW), ptr(dskip), ptr(dz1), ptr(dz2), ptr(sums), ctx.act, N, C, HW, stream_ptr())
        else:
            call(f"ppea_bn_bwd_channel_{_suffix(z1)}", ptr(dy), ptr(z1), ptr(z2), stats, ptr(maskf), 1.0 / float(N * HW),
                 ptr(dskip), ptr(dz1), ptr(dz2), ptr(sums), ctx.act, N, C, HW, stream_ptr())
        dg1, db1, dg2, db2, dr1, dr2 = _bn_grads(ctx, sums, z2 is not None, dy)
        return (dz1, dg1, db1, None, None, dz2, dg2, db2, None, None, None, dr1, dr2, None, None, None, None, None, None, None)


def bn_act_channel(z1, bn1, z2=None, bn2=None, mask=None, r1=None, r2=None, r2_scale=1.0, act=ACT_NONE, skip=False,
                   dup=False, sums=None):
    """-> (y, stats [4,C] = mean1 | invstd1 | mean2 | invstd2 [, z1 for the residual use when `skip`] [, y again for its
    second consumer when `dup`]).  Updates the running statistics of bn1 / bn2."""
    return _BnActChannel.apply(z1, bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var, z2,
                               None if bn2 is None else bn2.weight, None if bn2 is None else bn2.bias,
                               None if bn2 is None else bn2.running_mean, None if bn2 is None else bn2.running_var,
                               mask, r1, r2, r2_scale, act, bn1.eps, bn1.momentum, skip, dup, sums)


class _BnActChannelNext(torch.autograd.Function):
    """End of one block + first BatchNorm of the next in one launch per direction (csrc/bn_fused.hip, bn_*_channel_next):
    y = mask * BN_A(z) + r1 + s * r2,  y2 = BN_B(y).  Bit-identical to _BnActChannel(z, A, ...) followed by
    _BnActChannel(y, B, skip=True)."""

    @staticmethod
    def forward(ctx, z, gA, bA, rmA, rvA, gB, bB, rmB, rvB, mask, r1, r2, r2_scale, eps, momentum, dup=False):
        z, (r1, r2), (gAf, bAf, gBf, bBf), maskf, (N, C, HW) = _bn_operands(z, (r1, r2), (gA, bA, gB, bB), mask)
        st = torch.empty(4, C, device=z.device, dtype=_F32)          # meanA | invstdA | meanB | invstdB
        y, y2 = torch.empty_like(z), torch.empty_like(z)
        call(f"ppea_bn_fwd_channel_next_{_suffix(z)}", ptr(z), _ptr_array((gAf, bAf, gBf, bBf)),
             _ptr_array((rmA, rvA, rmB, rvB, st[0], st[1], st[2], st[3])), float(eps), float(momentum), ptr(maskf),
             ptr(r1), ptr(r2), float(r2_scale), ptr(y), ptr(y2), N, C, HW, stream_ptr())
        ctx.save_for_backward(z, y, st, gAf, bAf, gBf, bBf, maskf)
        ctx.r2_scale = float(r2_scale)
        ctx.has = (r1 is not None, r2 is not None)
        ctx.pdt = (gA.dtype, bA.dtype, gB.dtype, bB.dtype)
        ctx.mark_non_differentiable(st)
        ctx.set_materialize_grads(False)
        if dup:                                              # y2 once more for its second consumer (see _BnActChannel)
            return y, y2, st, y2.detach()
        return y, y2, st

    @staticmethod
    def backward(ctx, dy, dy2, _dst, dy2b=None):
        z, y, st, gAf, bAf, gBf, bBf, maskf = ctx.saved_tensors
        N, C = z.shape[0], z.shape[1]
        HW = z.numel() // (N * C)
        _other_stream_grad(dy2b)
        if dy2 is None:
            dy2, dy2b = (dy2b, None) if dy2b is not None else (torch.zeros_like(z), None)
        dy2 = dy2.contiguous().to(z.dtype)
        dskip = None if dy is None else dy.contiguous().to(z.dtype)
        sums = torch.empty(4, C, device=z.device, dtype=_F32)
        dz, dyt = torch.empty_like(z), torch.empty_like(z)
        stats = _ptr_array((st[0], st[1], gAf, bAf, st[2], st[3], gBf, bBf))
        if dy2b is not None:
            dy2b = dy2b.contiguous().to(z.dtype)
            call(f"ppea_bn_bwd_channel_next_dup_{_suffix(z)}", ptr(dy2), ptr(dy2b), ptr(dskip), ptr(z),
                 ptr(y), stats, ptr(maskf), 1.0 / float(N * HW), ptr(dz), ptr(dyt), ptr(sums), N, C, HW, stream_ptr())
        else:
            call(f"ppea_bn_bwd_channel_next_{_suffix(z)}", ptr(dy2), ptr(dskip), ptr(z), ptr(y), stats, ptr(maskf),
                 1.0 / float(N * HW), ptr(dz), ptr(dyt), ptr(sums), N, C, HW, stream_ptr())
        n = ctx.needs_input_grad
        dgA = sums[1].to(ctx.pdt[0]) if n[1] else None
        dbA = sums[0].to(ctx.pdt[1]) if n[2] else None
        dgB = sums[3].to(ctx.pdt[2]) if n[5] else None
        dbB = sums[2].to(ctx.pdt[3]) if n[6] else None
        dr1 = dyt if ctx.has[0] else None
        dr2 = (dyt if ctx.r2_scale == 1.0 else dyt * ctx.r2_scale) if ctx.has[1] else None
        return (dz, dgA, dbA, None, None, dgB, dbB, None, None, None, dr1, dr2, None, None, None, None)


def bn_act_channel_next(z, bnA, bnB, mask=None, r1=None, r2=None, r2_scale=1.0, dup=False):
    """-> (y, y2, stats [4,C] = meanA | invstdA | meanB | invstdB [, y2 again for its second consumer when `dup`]).  Updates
    the running statistics of both BNs."""
    return _BnActChannelNext.apply(z, bnA.weight, bnA.bias, bnA.running_mean, bnA.running_var, bnB.weight, bnB.bias,
                                   bnB.running_mean, bnB.running_var, mask, r1, r2, r2_scale, bnA.eps, bnA.momentum, dup)


# ---------------------------------------------------------------------------------------------
# A2 across ranks: SyncBatchNorm on the fused kernels (csrc/bn_sync.hip) -- two launches around ONE collective per
# BatchNorm and direction                                                   networks/replknet_adapter.py:170-180
# ---------------------------------------------------------------------------------------------
SYNC_COUNTERS = None      # bench.py / tests: {"launches": n, "collectives": m} accumulated while set to a dict


def _count(launches=0, collectives=0):
    if SYNC_COUNTERS is not None:
        SYNC_COUNTERS["launches"] = SYNC_COUNTERS.get("launches", 0) + launches
        SYNC_COUNTERS["collectives"] = SYNC_COUNTERS.get("collectives", 0) + collectives


def sync_bn_supported(z):
    return (z.is_cuda and z.dim() == 4 and z.dtype in (_F32, _BF16) and (z.shape[2] * z.shape[3]) % 8 == 0)


def sync_world(group):
    return dist.get_world_size(group)


def sync_rank(group):
    return dist.get_rank(group)


def gather_rows(table, group):
    """ONE all-gather, IN PLACE: `table` [world, pitch] arrives with this rank's row filled (the statistics kernel wrote
    straight into it) and leaves with every rank's row -- no staging copy on either side of the collective."""
    mine = table[sync_rank(group)]
    log_collective("all_gather", table, group)
    if dist.get_backend(group) == "nccl":
        dist.all_gather_into_tensor(table, mine, group=group)
    else:
        dist.all_gather(list(table.unbind(0)), mine.clone(), group=group)     # gloo has no tensor form
    _count(collectives=1)


def reduce_sums(sums, group):
    """ONE in-place all-reduce (sum) of a BatchNorm backward's [3][C] sums."""
    log_collective("all_reduce", sums, group)
    dist.all_reduce(sums, group=group)
    _count(collectives=1)


class _SyncBnAct(torch.autograd.Function):
    """y = act(BN1(z1) [+ BN2(z2)]) [* mask[n]] [+ r1] [+ s * r2] with statistics of the GLOBAL batch.
    forward : local statistics in wire format written into this rank's row of the gather table (one launch; none when
              `table` comes from the previous BatchNorm's apply launch; a tiny one when the producing GEMM left partial
              `sums`) -> in-place all-gather -> combine + running statistics + apply in one launch (`emit`: that launch
              also leaves the local statistics of y in the next BatchNorm's table);
    backward: reduce -> all-reduce [3][C] -> apply (+ the gradient `z1` receives through its other use when `skip`).
              d gamma / d beta leave as (global sum) / world: what the reference's DDP mean of the per-rank LOCAL sums
              comes to (torch's SyncBatchNorm returns local grad_weight / grad_bias; trainer.py:215-222)."""

    @staticmethod
    def forward(ctx, z1, g1, b1, rm1, rv1, z2, g2, b2, rm2, rv2, mask, r1, r2, r2_scale, act, eps, momentum, group, table,
                sums, skip, emit, dup=False):
        z1_in = z1
        z1, (z2, r1, r2), (g1f, b1f, g2f, b2f), maskf, (N, C, HW) = _bn_operands(z1, (z2, r1, r2), (g1, b1, g2, b2), mask)
        sfx = _suffix(z1)
        dev = z1.device
        two = z2 is not None
        pitch = (4 if two else 2) * C + 1
        world, rank = sync_world(group), sync_rank(group)
        if table is None:
            table = torch.empty(world, pitch, device=dev, dtype=_F32)
            row = _ct.c_void_p(table.data_ptr() + 4 * pitch * rank)
            if sums is not None and isinstance(sums, tuple) == two:
                # producer-epilogue partial sums [C][P][2]; a pair fills the two halves of one row (the first call's count
                # lands on mean2[0] and is overwritten by the second call, which runs after it on the stream)
                for k, sk in enumerate(sums if two else (sums,)):
                    call("ppea_bn_sync_stats_from_sums_f32", ptr(sk.contiguous(), _F32), sk.shape[1], C, N * HW,
                         _ct.c_void_p(row.value + 8 * C * k), stream_ptr())
                _count(launches=2 if two else 1)
            else:
                nws = _abi.lib.ppea_bn_sync_stats_workspace_bytes(N, C, HW, int(two)) // 4
                ws = torch.empty(nws, device=dev, dtype=_F32) if nws else None
                call(f"ppea_bn_sync_stats_{sfx}", ptr(z1), ptr(z2), row, ptr(ws), N, C, HW, stream_ptr())
                _count(launches=1 if not nws else (3 if two else 2))
        assert tuple(table.shape) == (world, pitch)
        gather_rows(table, group)
        st = torch.empty(4, C, device=dev, dtype=_F32)          # mean1 | invstd1 | mean2 | invstd2
        y = torch.empty_like(z1)
        nxt = torch.empty(world, 2 * C + 1, device=dev, dtype=_F32) if emit else None
        call(f"ppea_bn_sync_apply_{sfx}", ptr(z1), ptr(z2), ptr(table), world, _ptr_array((g1f, b1f, g2f, b2f)),
             _ptr_array((rm1, rv1, rm2, rv2, st[0], st[1], st[2], st[3])), float(eps), float(momentum), ptr(maskf), ptr(r1),
             ptr(r2), float(r2_scale), ptr(y), None if nxt is None else _ct.c_void_p(nxt.data_ptr() + 4 * (2 * C + 1) * rank),
             int(act), N, C, HW, stream_ptr())
        _count(launches=1)
        ctx.save_for_backward(z1, z2, st, g1f, b1f, g2f, b2f, maskf)
        ctx.act, ctx.r2_scale, ctx.group, ctx.world = int(act), float(r2_scale), group, world
        ctx.has = (r1 is not None, r2 is not None)
        ctx.pdt = (g1.dtype, b1.dtype, None if g2 is None else g2.dtype)
        ctx.skip, ctx.emit, ctx.dup = bool(skip), bool(emit), bool(dup)
        ctx.set_materialize_grads(False)
        outs = [y, st]
        ctx.mark_non_differentiable(st)
        if skip:
            outs.append(z1_in)
        if emit:
            outs.append(nxt)
            ctx.mark_non_differentiable(nxt)
        if dup:
            outs.append(y.detach())      # y again (same storage) for its second consumer: see _BnActChannel
        return tuple(outs)

    @staticmethod
    def backward(ctx, dy, _dst, *rest):
        z1, z2, st, g1f, b1f, g2f, b2f, maskf = ctx.saved_tensors
        N, C = z1.shape[0], z1.shape[1]
        HW = z1.numel() // (N * C)
        sfx = _suffix(z1)
        dev = z1.device
        if dy is None:
            dy = torch.zeros_like(z1)
        dy = dy.contiguous().to(z1.dtype)
        rest = list(rest)
        dskip = rest.pop(0) if ctx.skip else None
        if ctx.emit:
            rest.pop(0)
        dyb = rest.pop(0) if ctx.dup else None
        if dskip is not None:
            dskip = dskip.contiguous().to(z1.dtype)
        _other_stream_grad(dyb)
        if dyb is not None and (ctx.has[0] or ctx.has[1]):
            dy, dyb = dy + dyb.to(z1.dtype), None             # (r1 / r2 receive dy itself: not a block's first BatchNorm)
        two = z2 is not None
        stats = _ptr_array((st[0], st[1], g1f, b1f, st[2] if two else None, st[3] if two else None, g2f, b2f))
        sums, dy, final = _bn_bwd_sums(dy, z1, z2, stats, maskf, ctx.act, dyb)
        _count(launches=1 if final else 2)
        reduce_sums(sums, ctx.group)                            # -> sums of the global batch
        dz1 = torch.empty_like(z1)
        dz2 = torch.empty_like(z2) if two else None
        dgb = torch.empty(3, C, device=dev, dtype=_F32)         # d beta | d gamma1 | d gamma2, already divided by world
        call(f"ppea_bn_sync_bwd_apply_{sfx}", ptr(dy), ptr(z1), ptr(z2), stats, ptr(maskf), ptr(sums),
             1.0 / float(N * HW * ctx.world), ptr(dskip), ptr(dz1), ptr(dz2), ptr(dgb), 1.0 / ctx.world, ctx.act, N, C, HW,
             stream_ptr())
        _count(launches=1)
        dg1, db1, dg2, db2, dr1, dr2 = _bn_grads(ctx, dgb, two, dy)
        return (dz1, dg1, db1, None, None, dz2, dg2, db2, None, None, None, dr1, dr2) + (None,) * 10


def sync_bn_act(z1, bn1, z2=None, bn2=None, mask=None, r1=None, r2=None, r2_scale=1.0, act=ACT_NONE, group=None,
                table=None, sums=None, skip=False, emit=False, dup=False):
    """-> (y, stats [4,C] = mean1 | invstd1 | mean2 | invstd2 of the global batch [, z1 for the residual use when `skip`]
    [, the next BatchNorm's gather table with this rank's statistics of y filled in when `emit`] [, y again for its second
    consumer when `dup`]).  `table`: such a table
    from the launch that produced z1.  Updates the running statistics of bn1 / bn2."""
    return _SyncBnAct.apply(z1, bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var, z2,
                            None if bn2 is None else bn2.weight, None if bn2 is None else bn2.bias,
                            None if bn2 is None else bn2.running_mean, None if bn2 is None else bn2.running_var,
                            mask, r1, r2, r2_scale, act, bn1.eps, bn1.momentum, group, table, sums, skip, emit, dup)


def bn_act_apply(z1, g1, b1, mean1, invstd1, z2=None, g2=None, b2=None, mean2=None, invstd2=None, mask=None,
                 r1=None, r2=None, r2_scale=1.0, act=ACT_NONE, count=None, group=None):
    if count is None:
        count = z1.numel() // z1.shape[1]
    return _BnAct.apply(z1, g1, b1, mean1, invstd1, z2, g2, b2, mean2, invstd2, mask, r1, r2, r2_scale, act, count,
                        group)


# ---------------------------------------------------------------------------------------------
# pose trunk: training-mode BN (+ReLU, + residual before the activation) on channels_last tensors, per sub-batch
# ---------------------------------------------------------------------------------------------
def _raw(t, byte_offset=0):
    return None if t is None else _ct.c_void_p(t.data_ptr() + byte_offset)


def nhwc_bn_supported(x, groups=1):
    if not (x.is_cuda and x.dim() == 4 and x.dtype in (_F32, _BF16)):
        return False
    N, C = x.shape[0], x.shape[1]
    ct = C // 8
    return (C % 8 == 0 and 1 <= ct <= 256 and 256 % ct == 0 and N % groups == 0
            and x.is_contiguous(memory_format=torch.channels_last))


class _NhwcBnAct(torch.autograd.Function):
    """y = act(BN_g(x) + res) with separate batch statistics for each of `groups` consecutive sub-batches; the
    running statistics are updated once per sub-batch, in order.  Returns (y, stats [G,3,C]) with stats =
    mean | invstd | unbiased variance per sub-batch."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, res, act, groups, eps, momentum):
        N, C, H, W = x.shape
        P = (N // groups) * H * W
        sfx = _suffix(x)
        dev = x.device
        gam, bet = weight.detach().float().contiguous(), bias.detach().float().contiguous()
        slabs = _abi.lib.ppea_nhwc_bn_slabs(P, C)
        partial = torch.empty(groups * slabs * 2 * C, device=dev, dtype=_F32)
        stats = torch.empty(groups, 3, C, device=dev, dtype=_F32)
        ab = torch.empty(groups, 2, C, device=dev, dtype=_F32)
        y = torch.empty_like(x)                             # preserves channels_last
        st = stream_ptr()
        call(f"ppea_nhwc_bn_stats_{sfx}", _raw(x), ptr(partial), P, C, groups, st)
        call("ppea_nhwc_bn_finalize_f32", ptr(partial), P, C, groups, ptr(gam), ptr(bet), float(eps), float(momentum),
             ptr(stats), ptr(ab), ptr(running_mean), ptr(running_var), st)
        call(f"ppea_nhwc_bn_apply_{sfx}", _raw(x), _raw(res), ptr(ab), _raw(y), P, C, groups, int(act), st)
        ctx.save_for_backward(x, res, stats, ab)
        ctx.cfg = (int(act), int(groups), P, C, weight.dtype, bias.dtype)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)
        return y, stats

    @staticmethod
    def backward(ctx, dy, _ds):
        x, res, stats, ab = ctx.saved_tensors
        act, groups, P, C, wdt, bdt = ctx.cfg
        sfx = _suffix(x)
        dev = x.device
        if dy is None:
            dy = torch.zeros_like(x)
        dy = dy.contiguous(memory_format=torch.channels_last).to(x.dtype)
        slabs = _abi.lib.ppea_nhwc_bn_slabs(P, C)
        partial = torch.empty(groups * slabs * 2 * C, device=dev, dtype=_F32)
        kk = torch.empty(groups, 2, C, device=dev, dtype=_F32)
        tot = torch.empty(2, C, device=dev, dtype=_F32)
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if res is not None else None
        st = stream_ptr()
        call(f"ppea_nhwc_bn_bwd_reduce_{sfx}", _raw(x), _raw(dy), _raw(res), ptr(stats), ptr(ab), ptr(partial),
             P, C, groups, act, st)
        call("ppea_nhwc_bn_bwd_finalize_f32", ptr(partial), P, C, groups, ptr(kk), ptr(tot), st)
        call(f"ppea_nhwc_bn_bwd_apply_{sfx}", _raw(x), _raw(dy), _raw(res), ptr(stats), ptr(ab), ptr(kk),
             _raw(dx), _raw(dres), P, C, groups, act, st)
        return dx, tot[0].to(wdt), tot[1].to(bdt), None, None, dres, None, None, None, None


def nhwc_bn_act(x, weight, bias, running_mean, running_var, res=None, act=ACT_NONE, groups=1, eps=1e-5, momentum=0.1):
    return _NhwcBnAct.apply(x, weight, bias, running_mean, running_var, res, act, groups, eps, momentum)


# ---------------------------------------------------------------------------------------------
# pose trunk: MaxPool2d(3, 2, 1) on channels_last tensors (csrc/nhwc_pool.hip)          resnet_encoder.py:376-392
# ---------------------------------------------------------------------------------------------
class _MaxPoolNhwc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        N, C, H, W = x.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty(N, C, Ho, Wo, device=x.device, dtype=x.dtype, memory_format=torch.channels_last)
        idx = torch.empty(N, Ho, Wo, C, device=x.device, dtype=torch.uint8)
        call(f"ppea_nhwc_maxpool3x3s2_fwd_{_suffix(x)}", _raw(x), _raw(y), ptr(idx), N, H, W, C, stream_ptr())
        ctx.save_for_backward(idx)
        ctx.dims = (N, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        N, C, H, W = ctx.dims
        dy = dy.contiguous(memory_format=torch.channels_last)
        dx = torch.empty(N, C, H, W, device=dy.device, dtype=dy.dtype, memory_format=torch.channels_last)
        call(f"ppea_nhwc_maxpool3x3s2_bwd_{_suffix(dy)}", _raw(dy), ptr(idx), _raw(dx), N, H, W, C, stream_ptr())
        return dx


def maxpool3x3s2(x):
    """nn.MaxPool2d(3, 2, 1)(x) for a channels_last HIP tensor (C % 8 == 0, fp32 / bf16) on the gather kernels; None when
    this call is not served."""
    # (a 1 x 1 map is channels_last and NCHW-contiguous at once: same bytes, served)
    if not (x.is_cuda and x.dim() == 4 and x.dtype in (_F32, _BF16) and x.shape[1] % 8 == 0
            and x.is_contiguous(memory_format=torch.channels_last)):
        return None
    return _MaxPoolNhwc.apply(x)


# ---------------------------------------------------------------------------------------------
# A12 glue: bias + ELU of ConvBlock                                         layers.py:103-116
# ---------------------------------------------------------------------------------------------
def _is_nhwc(t):
    """channels_last storage (and not at the same time NCHW-contiguous, as C == 1 or H == W == 1 would be)."""
    return t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)


def _nhwc_c_ok(C):
    ct = C // 8
    return C % 8 == 0 and 1 <= ct <= 256 and 256 % ct == 0


class _BiasEluNhwc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, bias):
        N, C, H, W = z.shape
        y = torch.empty_like(z)
        bp, bflag = _bias_arg(bias.detach().contiguous())
        call(f"ppea_nhwc_bias_elu_fwd_{_suffix(z)}", _raw(z), bp, bflag, _raw(y), N * H * W, C, stream_ptr())
        ctx.save_for_backward(y)
        ctx.bdt = bias.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        N, C, H, W = y.shape
        dy = dy.contiguous(memory_format=torch.channels_last).to(y.dtype)
        slabs = _abi.lib.ppea_nhwc_bias_elu_slabs(N * H * W, C)
        partial = torch.empty(slabs, C, device=y.device, dtype=_F32)
        dz = torch.empty_like(y)
        call(f"ppea_nhwc_bias_elu_bwd_{_suffix(y)}", _raw(dy), _raw(y), _raw(dz), ptr(partial), N * H * W, C,
             stream_ptr())
        return dz, partial.sum(0).to(ctx.bdt)


class _BiasElu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, bias):
        z = z.contiguous()
        N, C = z.shape[0], z.shape[1]
        HW = z.numel() // (N * C)
        y = torch.empty_like(z)
        bp, bflag = _bias_arg(bias.detach().contiguous())
        call(f"ppea_bias_elu_fwd_{_suffix(z)}", ptr(z), bp, bflag, ptr(y), N, C, HW, stream_ptr())
        ctx.save_for_backward(y)
        ctx.bdt = bias.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        N, C = y.shape[0], y.shape[1]
        HW = y.numel() // (N * C)
        dy = dy.contiguous().to(y.dtype)
        chunks = _abi.lib.ppea_bias_elu_chunks(N, C, HW)
        partial = torch.empty(N, C, chunks, device=y.device, dtype=_F32)
        dz = torch.empty_like(y)
        call(f"ppea_bias_elu_bwd_{_suffix(y)}", ptr(dy), ptr(y), ptr(dz), ptr(partial), N, C, HW, stream_ptr())
        return dz, partial.sum((0, 2)).to(ctx.bdt)


def bias_elu(z, bias):
    """elu(z + bias[None, :, None, None]) in one pass; the bias gradient comes out of the backward pass.
    NCHW or channels_last input (output in the same format)."""
    if _is_nhwc(z):
        if _nhwc_c_ok(z.shape[1]):
            return _BiasEluNhwc.apply(z, bias)
        # a channel count the channels_last kernel does not serve: the NCHW kernel, the result handed back in the input's format
        return _BiasElu.apply(z, bias).contiguous(memory_format=torch.channels_last)
    return _BiasElu.apply(z, bias)


# ---------------------------------------------------------------------------------------------
# A12 glue: ReflectionPad2d(1)                                            layers.py:119-135
# ---------------------------------------------------------------------------------------------
class _ReflectPad1Nhwc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, C, H, W = x.shape
        out = torch.empty(B, C, H + 2, W + 2, device=x.device, dtype=x.dtype, memory_format=torch.channels_last)
        call(f"ppea_nhwc_reflect_pad1_fwd_{_suffix(x)}", _raw(x), _raw(out), B, H, W, C, stream_ptr())
        ctx.shape = (B, C, H, W)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, C, H, W = ctx.shape
        dout = dout.contiguous(memory_format=torch.channels_last)
        dx = torch.empty(B, C, H, W, device=dout.device, dtype=dout.dtype, memory_format=torch.channels_last)
        call(f"ppea_nhwc_reflect_pad1_bwd_{_suffix(dout)}", _raw(dout), _raw(dx), B, H, W, C, stream_ptr())
        return dx


class _ReflectPad1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        B, C, H, W = x.shape
        out = torch.empty(B, C, H + 2, W + 2, device=x.device, dtype=x.dtype)
        call(f"ppea_reflect_pad1_fwd_{_suffix(x)}", ptr(x), ptr(out), B * C, H, W, stream_ptr())
        ctx.shape = (B, C, H, W)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, C, H, W = ctx.shape
        dout = dout.contiguous()
        din = torch.empty(B, C, H, W, device=dout.device, dtype=dout.dtype)
        call(f"ppea_reflect_pad1_bwd_{_suffix(dout)}", ptr(dout), ptr(din), B * C, H, W, stream_ptr())
        return din


def reflect_pad1(x):
    if x.shape[-1] < 3 or x.shape[-2] < 3 or x.dtype not in (_F32, _BF16) or not x.is_cuda:
        return torch.nn.functional.pad(x, (1, 1, 1, 1), mode="reflect")
    if _is_nhwc(x) and x.shape[1] % 8 == 0:
        return _ReflectPad1Nhwc.apply(x)
    return _ReflectPad1.apply(x)


# ---------------------------------------------------------------------------------------------
# depthwise 3x3 (stride 1 / 2, pad 1) of the stem and the stage transitions   rka.py:414-416, 451-453
# ---------------------------------------------------------------------------------------------
class _DwConv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride):
        x = x.contiguous()
        N, C, H, W = x.shape
        wf = w.detach().to(_F32).contiguous()
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        y = torch.empty(N, C, Ho, Wo, device=x.device, dtype=x.dtype)
        call(f"ppea_dwconv3x3_fwd_{_suffix(x)}", ptr(x), ptr(wf), ptr(y), N, C, H, W, stride, stream_ptr())
        # (the input is kept only for a trainable filter: full fine-tuning)
        ctx.save_for_backward(wf, x if ctx.needs_input_grad[1] else None)
        ctx.meta = (N, C, H, W, stride, x.dtype, w.shape, w.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        wf, x = ctx.saved_tensors
        N, C, H, W, stride, dt, w_shape, w_dtype = ctx.meta
        dy = dy.contiguous().to(dt)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(N, C, H, W, device=dy.device, dtype=dt)
            call(f"ppea_dwconv3x3_bwd_data_{_suffix(dy)}", ptr(dy), ptr(wf), ptr(dx), N, C, H, W, stride, stream_ptr())
        if ctx.needs_input_grad[1]:
            nbytes = _abi.lib.ppea_dwconv3x3_bwd_filter_workspace_bytes(N, C, H, W, stride)
            if nbytes < 0:
                raise PpeaKernelError(f"dwconv3x3 filter gradient: shape {(N, C, H, W)} stride {stride} is not served")
            ws = torch.empty(nbytes // 4, device=dy.device, dtype=_F32)
            dw = torch.empty(w_shape, device=dy.device, dtype=_F32)
            call(f"ppea_dwconv3x3_bwd_filter_{_suffix(dy)}", ptr(x), ptr(dy), ptr(dw), ptr(ws), N, C, H, W, stride,
                 stream_ptr())
            dw = dw.to(w_dtype)
        return dx, dw, None


def dwconv3x3(x, w, stride):
    """Depthwise 3x3 (stride 1 / 2, pad 1, no bias) on the stencil kernels.  A frozen filter (the adapter configurations,
    repdepth.py:47-50) gets no gradient; a trainable one (--fullft_reb) gets it from ppea_dwconv3x3_bwd_filter_*."""
    return _DwConv3x3.apply(x, w, stride)


# ---------------------------------------------------------------------------------------------
# A5/A6  pointwise conv on MFMA (frozen 1x1 convs: forward with W, data gradient with W^T)
# ---------------------------------------------------------------------------------------------
def _pw_matrices(w):
    """(W [Cout][Cin] bf16, W^T [Cin][Cout] bf16) of a frozen 1x1 conv weight."""
    def build(w):
        m = w.detach().reshape(w.shape[0], w.shape[1]).to(_BF16).contiguous()
        return m, m.t().contiguous()
    return _weight_image(w, "pw", build, cache_trainable=True)


def pwconv_raw(a_mat, x, bias=None):
    """Y[b] = A @ X[b] (+ bias) for x [B,K,H,W] bf16, A [M,K] bf16 -> [B,M,H,W]; None if unsupported."""
    B, K, H, W = x.shape
    M = a_mat.shape[0]
    y = torch.empty(B, M, H, W, device=x.device, dtype=_BF16)
    served = try_call("ppea_pwconv_bf16", ptr(a_mat, _BF16), ptr(x, _BF16), ptr(bias), ptr(y), B, M, K, H * W, stream_ptr())
    return y if served else None


def _pw_forward(a, x, want_sums):
    """pwconv_raw(a, x), or with want_sums (y, sums [M, P, 2]): the epilogue also leaves per-channel partial sums of the
    stored output, so the BatchNorm that follows needs no statistics pass (batchnorm.fused_bn_act(..., sums=...))."""
    if not want_sums:
        return pwconv_raw(a, x)
    B, K, H, W = x.shape
    M = a.shape[0]
    y = torch.empty(B, M, H, W, device=x.device, dtype=_BF16)
    P = _abi.lib.ppea_pwconv_stats_partials(B, M, K, H * W)
    sums = torch.empty(M, P, 2, device=x.device, dtype=_F32)
    call("ppea_pwconv_stats_bf16", ptr(a, _BF16), ptr(x, _BF16), None, ptr(y), ptr(sums), B, M, K, H * W, stream_ptr())
    return y, sums


def _pw_gate(x, w):
    """The shapes the 1x1 GEMM serves for a weight [Cout, Cin, 1, 1]."""
    B, K, H, W = x.shape
    return x.dtype == _BF16 and x.is_cuda and K % 32 == 0 and w.shape[0] % 32 == 0 and (H * W) % 8 == 0


class _PwConvFrozen(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, want_sums=False):
        a, ctx.at = _pw_matrices(w)
        out = _pw_forward(a, x.contiguous(), want_sums)
        if want_sums:
            ctx.mark_non_differentiable(out[1])
            ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, dy, _dsums=None):
        return pwconv_raw(ctx.at, dy.contiguous().to(_BF16)), None, None


def pwconv_frozen(x, w, want_sums=False):
    """1x1 conv with a frozen weight [Cout,Cin,1,1] on the MFMA kernel; None when the shape is not served
    (caller falls back to the library conv).  want_sums: -> (y, sums [Cout, P, 2]) with the per-channel partial
    (sum, sum of squares) of y for the BatchNorm that follows."""
    if not _pw_gate(x, w) or w.requires_grad:
        return None
    return _PwConvFrozen.apply(x, w, True) if want_sums else _PwConvFrozen.apply(x, w)


class _PwConvTrainable(torch.autograd.Function):
    """1x1 conv with a TRAINABLE weight on the bf16 GEMM (full fine-tuning): the forward launches of _PwConvFrozen on
    W [Cout][Cin] bf16 -- the parameter itself when it is stored in bf16, else an image built on THIS use (flat Adam
    updates the weight through raw pointers, so no image of it is ever cached) --, the data gradient on W^T built per
    use, the weight gradient from the split-K reduce kernel in the parameter's layout and dtype."""

    @staticmethod
    def forward(ctx, x, w, want_sums=False):
        a = w.detach().reshape(w.shape[0], w.shape[1])
        a = a if a.dtype == _BF16 and a.is_contiguous() else a.to(_BF16).contiguous()
        x = x.contiguous()
        ctx.save_for_backward(x, a)
        ctx.w_meta = (w.shape, _grad_dtype(w))
        out = _pw_forward(a, x, want_sums)
        if want_sums:
            ctx.mark_non_differentiable(out[1])
            ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, dy, _dsums=None):
        x, a = ctx.saved_tensors
        dy = dy.contiguous().to(_BF16)
        dx = pwconv_raw(a.t().contiguous(), dy) if ctx.needs_input_grad[0] else None
        dw = pwgrad_into(dy, x, *ctx.w_meta)[0] if ctx.needs_input_grad[1] else None
        return dx, dw, None


def pwconv_trainable(x, w, want_sums=False):
    """pwconv_frozen for a weight that takes a gradient: same shape conditions (None when the GEMM does not serve them:
    the caller keeps ops.Conv2d), same forward arithmetic, and x.grad / w.grad from the bf16 GEMM kernels."""
    if not _pw_gate(x, w) or w.dim() != 4 or w.shape[2:] != (1, 1):
        return None
    return _PwConvTrainable.apply(x, w, True) if want_sums else _PwConvTrainable.apply(x, w)


# ---------------------------------------------------------------------------------------------
# A4  adapters on the MFMA kernels, NCHW bf16 end to end (replknet_adapter.py:20-109)
# ---------------------------------------------------------------------------------------------
EPI_NONE, EPI_GELU, EPI_DGELU = 0, 1, 2


def _bias_arg(b):
    if b is None:
        return None, 0
    if b.dtype == _BF16:
        return ptr(b, _BF16), 1
    return ptr(b, _F32), 0


def pwconv_ex(a_mat, x, bias=None, epi=EPI_NONE, aux=None, transposed=False):
    """A [M,K] bf16 (or, with transposed=True, At [K,M]) applied over the channel axis of x [B,K,H,W] bf16 with
    an epilogue: EPI_NONE -> y;  EPI_GELU -> (pre, gelu(pre));  EPI_DGELU -> (A x) * gelu'(aux)."""
    B, K, H, W = x.shape
    M = a_mat.shape[1] if transposed else a_mat.shape[0]
    y = torch.empty(B, M, H, W, device=x.device, dtype=_BF16)
    y2 = torch.empty_like(y) if epi == EPI_GELU else None
    bp, bflag = _bias_arg(bias)
    call("ppea_pwconv_ex_bf16", ptr(a_mat, _BF16), ptr(x, _BF16), bp, bflag, epi, ptr(aux, _BF16) if aux is not None
         else None, ptr(y), ptr(y2), B, M, K, H * W, int(transposed), stream_ptr())
    return (y, y2) if epi == EPI_GELU else y


def pwgrad(p, q, want_rowsum=True):
    """(sum_{b,pixels} p[b,m,:] q[b,n,:]  [M,N] fp32,  sum_{b,pixels} p[b,m,:]  [M] fp32 or None)."""
    B, M, H, W = p.shape
    N = q.shape[1]
    ws = torch.empty(_abi.lib.ppea_pwgrad_workspace_bytes(B, M, N, H * W) // 4, device=p.device, dtype=_F32)
    out = torch.empty(M * N + M, device=p.device, dtype=_F32)
    call("ppea_pwgrad_bf16", ptr(p, _BF16), ptr(q, _BF16), ptr(out), ptr(ws), B, M, N, H * W, int(want_rowsum),
         stream_ptr())
    return out[:M * N].view(M, N), (out[M * N:] if want_rowsum else None)


def pwgrad_into(p, q, w_shape, w_dtype, taps=1, b_rows=None, b_dtype=None):
    """Weight (and bias) gradients written straight in parameter layout / dtype by the reduce kernel:
    dW = sum_{b,pixels} p[b,m,:] q[b,n,:] as `w_shape` (taps = 9: p rows are tap-major, dW in Conv2d layout);
    db = row sums of p rows `b_rows` = (first, count)."""
    B, M, H, W = p.shape
    N = q.shape[1]
    ws = torch.empty(_abi.lib.ppea_pwgrad_workspace_bytes(B, M, N, H * W) // 4, device=p.device, dtype=_F32)
    dw = torch.empty(w_shape, device=p.device, dtype=w_dtype)
    db = torch.empty(b_rows[1], device=p.device, dtype=b_dtype) if b_rows is not None else None
    call("ppea_pwgrad_ex_bf16", ptr(p, _BF16), ptr(q, _BF16), ptr(ws), B, M, N, H * W, ptr(dw), int(w_dtype == _BF16),
         taps, ptr(db), int(b_dtype == _BF16), b_rows[0] if b_rows else 0, b_rows[1] if b_rows else 0, stream_ptr())
    return dw, db


PWGRAD_PAIR = os.environ.get("PPEA_PWGRAD_PAIR", "1") == "1"


def pwgrad_into_pair(a, b):
    """Two pwgrad_into problems over the same pixels -- a, b = (p, q, w_shape, w_dtype, taps, b_rows, b_dtype) -- in ONE GEMM
    launch and ONE reduce launch (an adapter's D_fc2 and D_fc1 weight gradients); falls back to two calls where the pair
    form is not served.  -> ((dw_a, db_a), (dw_b, db_b))."""
    (pa, qa), (pb, qb) = a[:2], b[:2]
    B, _, H, W = pa.shape
    if PWGRAD_PAIR and pb.shape[0] == B and pb.shape[2:] == pa.shape[2:]:
        Ms = (_ct.c_int * 2)(pa.shape[1], pb.shape[1])
        Ns = (_ct.c_int * 2)(qa.shape[1], qb.shape[1])
        nbytes = _abi.lib.ppea_pwgrad_pair_workspace_bytes(B, Ms, Ns, H * W)
        if nbytes > 0:
            dev = pa.device
            ws = torch.empty(nbytes // 4, device=dev, dtype=_F32)
            outs = []
            for (_p, _q, w_shape, w_dtype, taps, b_rows, b_dtype) in (a, b):
                outs.append((torch.empty(w_shape, device=dev, dtype=w_dtype),
                             torch.empty(b_rows[1], device=dev, dtype=b_dtype) if b_rows is not None else None))
            i2 = _ct.c_int * 2

            def vp2(u, v, dt=None):                       # array of two device pointers (None -> NULL)
                return (_ct.c_void_p * 2)(*(None if t_ is None else ptr(t_, dt).value for t_ in (u, v)))
            rows = [x[5] if x[5] is not None else (0, 0) for x in (a, b)]
            call("ppea_pwgrad_ex_pair_bf16", vp2(pa, pb, _BF16), vp2(qa, qb, _BF16), ptr(ws), B,
                 Ms, Ns, H * W, vp2(outs[0][0], outs[1][0]), i2(int(a[3] == _BF16), int(b[3] == _BF16)),
                 i2(a[4], b[4]), vp2(outs[0][1], outs[1][1]), i2(int(a[6] == _BF16), int(b[6] == _BF16)),
                 i2(rows[0][0], rows[1][0]), i2(rows[0][1], rows[1][1]), stream_ptr())
            return outs[0], outs[1]
    return pwgrad_into(*a), pwgrad_into(*b)


class _PoseMatrix(torch.autograd.Function):
    """A15 `transformation_from_parameters` (layers.py:26-42, 61-100): axis-angle [B,3] + translation [B,3] -> [B,4,4], one
    launch forward and one backward (exact Jacobian) instead of ~25 + ~50 tiny element-wise kernels on the step's stream."""

    @staticmethod
    def forward(ctx, aa, tr, invert):
        aa, tr = aa.contiguous(), tr.contiguous()
        B = aa.shape[0]
        T = torch.empty(B, 4, 4, device=aa.device, dtype=_F32)
        call("ppea_pose_matrix_fwd_f32", ptr(aa, _F32), ptr(tr, _F32), ptr(T), B, int(invert), stream_ptr())
        ctx.save_for_backward(aa, tr)
        ctx.invert = int(invert)
        return T

    @staticmethod
    def backward(ctx, dT):
        aa, tr = ctx.saved_tensors
        B = aa.shape[0]
        daa, dtr = torch.empty_like(aa), torch.empty_like(tr)
        call("ppea_pose_matrix_bwd_f32", ptr(aa), ptr(tr), ptr(dT.contiguous().float()), ptr(daa), ptr(dtr), B, ctx.invert,
             stream_ptr())
        return daa, dtr, None


def pose_matrix(axisangle, translation, invert=False):
    """axisangle, translation [B,1,3] (or [B,3]) fp32 on the device -> [B,4,4] fp32."""
    return _PoseMatrix.apply(axisangle.reshape(-1, 3).float(), translation.reshape(-1, 3).float(), bool(invert))


POSE_CHAIN_MAX = 4        # csrc/geometry.hip POSE_CHAIN_MAX: lookup frames and pose-network outputs per launch


def _pose_rows(ts, B):
    """Pose-decoder outputs [B,1,3] or [B,3] as the chain kernels read them -> ([B,3] tensors, floats from one item to the
    next).  Views that are fp32 on the device, dense in their last axis and share one batch stride (slices of the decoder's
    output) are read in place; anything else is copied to contiguous fp32 [B,3]."""
    rows = [t.reshape(B, 3) for t in ts]                          # views: [B,1,3] -> [B,3] keeps the batch stride
    stride = rows[0].stride(0) if B > 1 else 3
    if all(t.is_cuda and t.dtype == _F32 and t.stride(1) == 1 and (B <= 1 or t.stride(0) == stride) and stride >= 3
           for t in rows):
        return rows, stride
    return [t.float().contiguous() for t in rows], 3


@torch.no_grad()
def pose_chain(pairs, chain, keep=None):
    """Relative poses of the F lookup frames in one launch (repdepth.py:465-507; no gradient, as in the reference).
    pairs: P <= 4 pose-network outputs (axisangle, translation), each [B,1,3] or [B,3] on the device (views with a
    batch stride are read in place); chain: per frame (index into `pairs`, invert, index of the predecessor FRAME in
    `chain` or -1), predecessors first; keep: [B,F], zero = that (item, frame) is written as exact zeros and so is every
    frame chained behind it (None: keep all).  -> [B,F,4,4] fp32, T(f) = T_pair(f) @ T(pred(f))."""
    P, Fr = len(pairs), len(chain)
    if not (1 <= P <= POSE_CHAIN_MAX and 1 <= Fr <= POSE_CHAIN_MAX):
        raise PpeaKernelError(f"pose_chain serves 1..{POSE_CHAIN_MAX} pairs and frames, got {P} and {Fr}")
    for f, (p, _inv, pred) in enumerate(chain):
        if not (0 <= p < P and -1 <= pred < f):
            raise PpeaKernelError(f"pose_chain: frame {f} names pair {p} / predecessor {pred}")
    B = pairs[0][0].shape[0]
    flat, stride = _pose_rows([t for pr in pairs for t in pr], B)
    dev = flat[0].device
    for t in flat:
        if not t.is_cuda or t.device != dev:
            raise PpeaKernelError("PPEA-Depth HIP kernels need tensors on a HIP device (no CPU fallback)")
    keep = None if keep is None else keep.to(_F32).contiguous()
    if keep is not None and keep.shape != (B, Fr):
        raise PpeaKernelError(f"pose_chain: keep {tuple(keep.shape)} for B = {B}, F = {Fr}")
    if keep is not None and keep.device != dev:
        raise PpeaKernelError("pose_chain: keep is on another device")
    T = torch.empty(B, Fr, 4, 4, device=dev, dtype=_F32)
    vps, ints = _ct.c_void_p * P, _ct.c_int * Fr
    call("ppea_pose_chain_fwd_f32", vps(*(t.data_ptr() for t in flat[0::2])), vps(*(t.data_ptr() for t in flat[1::2])), P,
         stride, ints(*(c[0] for c in chain)), ints(*(int(bool(c[1])) for c in chain)), ints(*(c[2] for c in chain)),
         ptr(keep), ptr(T), B, Fr, stream_ptr())
    return T


@torch.no_grad()
def pose_chain_ring(ring, state, new=None):
    """The relative poses of a video stream's lookup frames -1 .. -F from the pose ring [F,B,2,3] fp32 (slot (head - j) mod F:
    the pose decoder's raw (axisangle, translation) of the pair (t-j-1, t-j)) in one launch.  new = (axisangle, translation)
    [B,1,3] or [B,3] of the pair (t-1, t): stored into slot head by the same launch (None: it is there already).
    -> (T [B,F,4,4] = `pose_chain`'s on those pairs, exact zeros where seen[b] <= j; present [B,F] bool)."""
    Fr, B = ring.shape[:2]
    if ring.dtype != _F32 or tuple(ring.shape[2:]) != (2, 3) or not 1 <= Fr <= POSE_CHAIN_MAX:
        raise PpeaKernelError(f"pose_chain_ring: ring {ring.dtype} {tuple(ring.shape)}, expected fp32 [1..{POSE_CHAIN_MAX},B,2,3]")
    if state.dtype != torch.int32 or state.shape != (1 + B,) or state.device != ring.device:
        raise PpeaKernelError(f"stream state must be int32 [1 + {B}] on {ring.device}")
    aa = tr = None
    stride = 3
    if new is not None:
        (aa, tr), stride = _pose_rows(new, B)
        if aa.device != ring.device or tr.device != ring.device:
            raise PpeaKernelError("pose_chain_ring: the new pair is on another device")
    T = torch.empty(B, Fr, 4, 4, device=ring.device, dtype=_F32)
    present = torch.empty(B, Fr, device=ring.device, dtype=torch.uint8)
    call("ppea_pose_chain_ring_fwd_f32", None if aa is None else _ct.c_void_p(aa.data_ptr()),
         None if tr is None else _ct.c_void_p(tr.data_ptr()), stride, ptr(ring), ptr(state), ptr(T), ptr(present), B, Fr,
         stream_ptr())
    return T, present.view(torch.bool)


def tapsum_fwd(T, bias, Ch):
    B, _, H, W = T.shape
    pre = torch.empty(B, Ch, H, W, device=T.device, dtype=_BF16)
    h = torch.empty_like(pre)
    bp, bflag = _bias_arg(bias)
    call("ppea_tapsum_fwd_bf16", ptr(T, _BF16), bp, bflag, ptr(pre), ptr(h), B, Ch, H, W, stream_ptr())
    return pre, h


def tapsum_bwd(g):
    B, Ch, H, W = g.shape
    dT = torch.empty(B, 9 * Ch, H, W, device=g.device, dtype=_BF16)
    call("ppea_tapsum_bwd_bf16", ptr(g, _BF16), ptr(dT), B, Ch, H, W, stream_ptr())
    return dT


def adapter_supported(x, hidden):
    """Any hidden width is served: mlp_adapter / conv_adapter zero-pad it to the next multiple of 32 (RepLKNet-31L stage 0:
    hidden 48; the Stage-2 decoder adapter: 148)."""
    B, C, H, W = x.shape
    return (x.is_cuda and x.dtype == _BF16 and C % 32 == 0 and hidden >= 1 and (H * W) % 8 == 0 and W % 4 == 0)


def _pad_hidden(w1, b1, w2):
    """Zero rows for D_fc1 / zero columns for D_fc2 up to a hidden width the GEMM kernels take (a multiple of 32).  The
    padded units compute gelu(0) = 0 and meet zero columns: same function, same gradients (autograd slices the padded
    gradients back); three small concatenations per call."""
    Ch = w1.shape[0]
    pad = (-Ch) % 32
    if pad == 0:
        return w1, b1, w2
    w1p = torch.cat([w1, w1.new_zeros((pad,) + tuple(w1.shape[1:]))], 0)
    b1p = None if b1 is None else torch.cat([b1, b1.new_zeros(pad)], 0)
    w2p = torch.cat([w2, w2.new_zeros(w2.shape[0], pad)], 1)
    return w1p, b1p, w2p


def _grad_dtype(t):
    return t.dtype if t.dtype in (_BF16, _F32) else _F32


class _MlpAdapterFn(torch.autograd.Function):
    """`Adapter` (rka.py:20-47): y = W2 gelu(W1 x + b1) + b2 over the channel axis.  No weight repacking: the
    data gradients consume the forward matrices through the kernel's transposed-A mode, and the weight / bias
    gradients leave the reduce kernel in parameter dtype."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        x = x.contiguous()
        w1m, w2m = w1.to(_BF16).contiguous(), w2.to(_BF16).contiguous()
        pre, h = pwconv_ex(w1m, x, b1, EPI_GELU)
        y = pwconv_ex(w2m, h, b2)
        ctx.save_for_backward(x, pre, h, w1m, w2m)
        ctx.dtypes = tuple(_grad_dtype(t) for t in (w1, b1, w2, b2))
        ctx.shapes = (w1.shape, w2.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, pre, h, w1m, w2m = ctx.saved_tensors
        t = ctx.dtypes
        C, Ch = w2m.shape
        dy = dy.contiguous()
        g = pwconv_ex(w2m, dy, None, EPI_DGELU, pre, transposed=True)          # W2^T dy: At = W2 [C][Ch]
        (dw2, db2), (dw1, db1) = pwgrad_into_pair((dy, h, ctx.shapes[1], t[2], 1, (0, C), t[3]),
                                                  (g, x, ctx.shapes[0], t[0], 1, (0, Ch), t[1]))
        dx = pwconv_ex(w1m, g, transposed=True) if ctx.needs_input_grad[0] else None
        return dx, dw1, db1, dw2, db2


class _ConvAdapterFn(torch.autograd.Function):
    """`B_Adapter`, adpt_test 4 (rka.py:49-109): y = W2 gelu(conv3x3(x; W1) + b1) + b2.  One repack per step
    (W1 -> tap-major [9*Ch][C]); its transpose for the data gradient is the kernel's transposed-A mode."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        x = x.contiguous()
        Ch, C = w1.shape[0], w1.shape[1]
        a1 = w1.to(_BF16).permute(2, 3, 0, 1).reshape(9 * Ch, C).contiguous()     # rows t*Ch + m
        w2m = w2.to(_BF16).contiguous()
        T = pwconv_ex(a1, x)
        pre, h = tapsum_fwd(T, b1, Ch)
        y = pwconv_ex(w2m, h, b2)
        ctx.save_for_backward(x, pre, h, a1, w2m)
        ctx.dtypes = tuple(_grad_dtype(t) for t in (w1, b1, w2, b2))
        ctx.shapes = (w1.shape, w2.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, pre, h, a1, w2m = ctx.saved_tensors
        t = ctx.dtypes
        C, Ch = w2m.shape
        dy = dy.contiguous()
        g = pwconv_ex(w2m, dy, None, EPI_DGELU, pre, transposed=True)
        dT = tapsum_bwd(g)
        (dw2, db2), (dw1, db1) = pwgrad_into_pair((dy, h, ctx.shapes[1], t[2], 1, (0, C), t[3]),
                                                  (dT, x, ctx.shapes[0], t[0], 9, (4 * Ch, Ch), t[1]))   # centre-tap rows == g
        dx = pwconv_ex(a1, dT, transposed=True) if ctx.needs_input_grad[0] else None  # At = a1 [9*Ch][C]
        return dx, dw1, db1, dw2, db2


def mlp_adapter(x, w1, b1, w2, b2):
    w1, b1, w2 = _pad_hidden(w1, b1, w2)
    return _MlpAdapterFn.apply(x, w1, b1, w2, b2)


def conv_adapter(x, w1, b1, w2, b2):
    w1, b1, w2 = _pad_hidden(w1, b1, w2)
    return _ConvAdapterFn.apply(x, w1, b1, w2, b2)


class _PwLinear(torch.autograd.Function):
    """y[b, :, p] = W x[b, :, p] (+ bias) over the channel axis of NCHW bf16 x with a TRAINABLE W [M, K]: forward and data
    gradient on pwconv (the data gradient consumes W through the kernel's transposed-A mode), weight / bias gradients on
    pwgrad, written in parameter dtype."""

    @staticmethod
    def forward(ctx, x, w, b):
        x = x.contiguous()
        wm = w.to(_BF16).contiguous()
        y = pwconv_ex(wm, x, b)
        ctx.save_for_backward(x, wm)
        ctx.meta = (tuple(w.shape), _grad_dtype(w), None if b is None else _grad_dtype(b))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wm = ctx.saved_tensors
        wshape, wdt, bdt = ctx.meta
        dy = dy.contiguous().to(_BF16)
        dx = pwconv_ex(wm, dy, transposed=True) if ctx.needs_input_grad[0] else None
        dw = db = None
        if ctx.needs_input_grad[1] or (bdt is not None and ctx.needs_input_grad[2]):
            dw, db = pwgrad_into(dy, x, wshape, wdt, 1, None if bdt is None else (0, wshape[0]), bdt)
        return dx, dw, db


def pw_linear_supported(x, M):
    B, K, H, W = x.shape
    return x.is_cuda and x.dtype == _BF16 and K % 32 == 0 and M % 8 == 0 and (H * W) % 8 == 0


def pw_linear(x, w, b=None):
    """nn.Linear(K -> M) over the channel axis of x [B,K,H,W] bf16 -> [B,M,H,W] (trainable weight and bias)."""
    return _PwLinear.apply(x, w, b)


# ---------------------------------------------------------------------------------------------
# fp32 dense convolutions / linear layers on the fp32 matrix cores (csrc/conv_f32.hip): the fp32 (parity, BASELINE config 1)
# step's replacement for the library convolution / GEMM behind every groups == 1 conv, nn.Linear and ConvTranspose2d of the
# path (rka.py:20-109, 264-326; depth_decoder_v2.py:172-245; resnet_encoder.py:367-409; pose_decoder.py:27-52).  Operands
# are addressed through element strides: NCHW and channels_last tensors go in as they are.
# ---------------------------------------------------------------------------------------------
CONV_F32_MFMA = True       # False: the library (tests compare the two)


def _strides(t):
    return (_ct.c_long * 4)(*[int(v) for v in t.stride()])


def _like_format(x, shape):
    cl = x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()
    return torch.empty(shape, device=x.device, dtype=_F32, memory_format=torch.channels_last if cl else torch.contiguous_format)


def _f32_dense(x):
    """A 4-D fp32 HIP tensor whose strides the kernels may use as they are (any dense or expanded layout)."""
    return x if all(st >= 0 for st in x.stride()) else x.contiguous()


def _gen_sfx(x):
    return "bf16" if x.dtype == _BF16 else "f32"


def _gen_out(x, shape):
    cl = x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()
    return torch.empty(shape, device=x.device, dtype=x.dtype, memory_format=torch.channels_last if cl else torch.contiguous_format)


def _f32_vec(b):
    return None if b is None else ptr(b.detach().float().contiguous(), _F32)


class _Conv2dF32(torch.autograd.Function):
    """x, w both fp32 or both bf16 (the caller casts); bias any float dtype (read as fp32)."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pad):
        x = _f32_dense(x)
        N, Cin, H, W = x.shape
        Cout, _, R, S = w.shape
        Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
        wd = w.detach().to(x.dtype).contiguous()
        y = _gen_out(x, (N, Cout, Ho, Wo))
        call(f"ppea_conv2d_{_gen_sfx(x)}_fwd", _raw(x), _strides(x), ptr(wd), _f32_vec(bias), _raw(y), _strides(y), N, Cin, H, W,
             Cout, R, S, stride, pad, stream_ptr())
        ctx.save_for_backward(x, wd)
        ctx.cfg = (stride, pad, Ho, Wo, None if bias is None else bias.dtype, w.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wd = ctx.saved_tensors
        stride, pad, Ho, Wo, bdt, wdt = ctx.cfg
        N, Cin, H, W = x.shape
        Cout, _, R, S = wd.shape
        dy = _f32_dense(dy.to(x.dtype))
        sfx = _gen_sfx(x)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _gen_out(x, x.shape)
            call(f"ppea_conv2d_{sfx}_dgrad", _raw(dy), _strides(dy), ptr(wd), _raw(dx), _strides(dx), N, Cin, H, W, Cout, R, S,
                 stride, pad, Ho, Wo, stream_ptr())
        if ctx.needs_input_grad[1]:
            nbytes = _abi.lib.ppea_conv2d_f32_wgrad_workspace_bytes(N, Cin, Cout, R, S, Ho, Wo)
            ws = torch.empty(nbytes // 4, device=x.device, dtype=_F32) if nbytes else None
            dw = torch.empty(Cout, Cin, R, S, device=x.device, dtype=_F32)
            call(f"ppea_conv2d_{sfx}_wgrad", _raw(x), _strides(x), _raw(dy), _strides(dy), ptr(dw), ptr(ws), N, Cin, H, W, Cout,
                 R, S, stride, pad, Ho, Wo, stream_ptr())
            dw = dw.to(wdt)
        if bdt is not None and ctx.needs_input_grad[2]:
            db = dy.float().sum((0, 2, 3)).to(bdt)
        return dx, dw, db, None, None


def conv2d_f32_ok(x, w, stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1, padding_mode="zeros"):
    """This call is served by csrc/conv_f32.hip: fp32 tensors outside autocast (the fp32 step), or bf16 activations (the bf16
    step's shapes that its layout-specialised kernels do not take)."""
    if not (CONV_F32_MFMA and x.is_cuda and x.dim() == 4 and groups == 1 and tuple(dilation) == (1, 1)
            and not isinstance(padding, str) and padding_mode == "zeros" and stride[0] == stride[1]
            and padding[0] == padding[1] and w.dtype in (_F32, _BF16)):
        return False
    if x.dtype == _BF16:
        return True
    return x.dtype == _F32 and w.dtype == _F32 and not torch.is_autocast_enabled()


def conv2d_f32(x, w, bias=None, stride=1, pad=0):
    """F.conv2d(x, w, bias, stride, pad), groups = 1, on the fp32 MFMA kernels (fp32, or bf16 storage with fp32 arithmetic)."""
    return _Conv2dF32.apply(x, w, bias, int(stride), int(pad))


def conv2d(x, w, bias=None, stride=1, pad=0):
    """Dense conv of the path: HIP tensors on this build's kernel, anything else through torch."""
    if conv2d_f32_ok(x, w, (stride, stride), (pad, pad)):
        return conv2d_f32(x, w, bias, stride, pad)
    return torch.nn.functional.conv2d(x, w, bias, stride, pad)


class Conv2d(torch.nn.Conv2d):
    """nn.Conv2d of this package: the bf16 step reaches the layout-specialised kernels through `conv_module` /
    `pwconv_frozen`; whatever falls through to `nn.Conv2d.forward` lands HERE -- HIP tensors run on csrc/conv_f32.hip (fp32
    step: every dense conv; bf16 step: shapes the specialised kernels refuse), everything else (CPU tensors) on torch."""

    def _conv_forward(self, input, weight, bias):
        if conv2d_f32_ok(input, weight, self.stride, self.padding, self.dilation, self.groups, self.padding_mode):
            return conv2d_f32(input, weight, bias, self.stride[0], self.padding[0])
        return super()._conv_forward(input, weight, bias)


def channel_linear_f32(x, w, b):
    """nn.Linear(K -> M) over the channel axis of x [B,K,H,W] = a 1x1 convolution."""
    return conv2d_f32(x, w.view(w.shape[0], w.shape[1], 1, 1), b, 1, 0)


class _ConvTransposeF32(torch.autograd.Function):
    """ConvTranspose2d (weight [Cin][Cout][R][S]) = the data gradient of the conv with that weight; its data gradient is that
    conv's forward and its weight gradient that conv's weight gradient with the two activations exchanged."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, out_pad):
        x = _f32_dense(x)
        N, Cin, H, W = x.shape
        _, Cout, R, S = w.shape
        Ho, Wo = (H - 1) * stride - 2 * pad + R + out_pad, (W - 1) * stride - 2 * pad + S + out_pad
        wd = w.detach().to(x.dtype).contiguous()
        y = _gen_out(x, (N, Cout, Ho, Wo))
        call(f"ppea_conv2d_{_gen_sfx(x)}_dgrad", _raw(x), _strides(x), ptr(wd), _raw(y), _strides(y), N, Cout, Ho, Wo, Cin, R, S,
             stride, pad, H, W, stream_ptr())
        if bias is not None:
            y += bias.detach().to(y.dtype).view(1, -1, 1, 1)
        ctx.save_for_backward(x, wd)
        ctx.cfg = (stride, pad, Ho, Wo, None if bias is None else bias.dtype, w.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wd = ctx.saved_tensors
        stride, pad, Ho, Wo, bdt, wdt = ctx.cfg
        N, Cin, H, W = x.shape
        _, Cout, R, S = wd.shape
        dy = _f32_dense(dy.to(x.dtype))
        sfx = _gen_sfx(x)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _gen_out(x, x.shape)
            call(f"ppea_conv2d_{sfx}_fwd", _raw(dy), _strides(dy), ptr(wd), None, _raw(dx), _strides(dx), N, Cout, Ho, Wo, Cin, R, S,
                 stride, pad, stream_ptr())
        if ctx.needs_input_grad[1]:
            nbytes = _abi.lib.ppea_conv2d_f32_wgrad_workspace_bytes(N, Cout, Cin, R, S, H, W)
            ws = torch.empty(nbytes // 4, device=x.device, dtype=_F32) if nbytes else None
            dw = torch.empty(Cin, Cout, R, S, device=x.device, dtype=_F32)
            call(f"ppea_conv2d_{sfx}_wgrad", _raw(dy), _strides(dy), _raw(x), _strides(x), ptr(dw), ptr(ws), N, Cout, Ho, Wo, Cin,
                 R, S, stride, pad, H, W, stream_ptr())
            dw = dw.to(wdt)
        if bdt is not None and ctx.needs_input_grad[2]:
            db = dy.float().sum((0, 2, 3)).to(bdt)
        return dx, dw, db, None, None, None


def conv_transpose_f32_module(m, x):
    """nn.ConvTranspose2d `m` on the fp32 MFMA kernels, or None when this call is not served."""
    if not (CONV_F32_MFMA and x.is_cuda and m.groups == 1 and tuple(m.dilation) == (1, 1) and m.stride[0] == m.stride[1]
            and m.padding[0] == m.padding[1] and m.output_padding[0] == m.output_padding[1]
            and m.kernel_size[0] == m.kernel_size[1] and m.weight.dtype in (_F32, _BF16)
            and (x.dtype == _BF16 or (x.dtype == _F32 and m.weight.dtype == _F32 and not torch.is_autocast_enabled()))):
        return None
    return _ConvTransposeF32.apply(x, m.weight, m.bias, m.stride[0], m.padding[0], m.output_padding[0])


# ---------------------------------------------------------------------------------------------
# A13  transposed convolution of the Stage-2 decoder adapter (depth_decoder_v2.py:137-139: ConvTranspose2d(c, c, 3, 2, 1,
# output_padding=1)) on the implicit-GEMM kernels: the forward IS the data gradient of a stride-2 conv, its data gradient is
# that conv's forward, its weight gradient that conv's weight gradient with the two activations exchanged.
# ---------------------------------------------------------------------------------------------
class _ConvTransposeNhwc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, out_pad):
        x = _as_nhwc(x)
        N, Cin, H, W = x.shape
        _, Cout, R, S = w.shape                                  # ConvTranspose2d weight: [Cin, Cout, R, S]
        Ho, Wo = (H - 1) * stride - 2 * pad + R + out_pad, (W - 1) * stride - 2 * pad + S + out_pad
        # as a conv weight [Cout_c = Cin][Cin_c = Cout][R][S]: the flipped / transposed operand image of its data gradient
        y = conv_nhwc_raw(x, _conv_packed(w, True), None if bias is None else bias.detach().contiguous(), Cout, R, S, 1,
                          R - 1 - pad, False, stride, Ho, Wo, 0, False)
        ctx.save_for_backward(x, w)
        ctx.cfg = (stride, pad, Ho, Wo, None if bias is None else bias.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, pad, Ho, Wo, bdt = ctx.cfg
        N, Cin, H, W = x.shape
        _, Cout, R, S = w.shape
        dz = _as_nhwc(dy.to(_BF16))
        db = dz.float().sum((0, 2, 3)).to(bdt) if (bdt is not None and ctx.needs_input_grad[2]) else None
        dx = dw = None
        if ctx.needs_input_grad[0]:                              # = conv2d(dy, w as [Cin][Cout][R][S], stride, pad)
            dx = conv_nhwc_raw(dz, _conv_packed(w, False), None, Cin, R, S, stride, pad, False, 1, H, W, 0, False)
        if ctx.needs_input_grad[1]:
            if Cin % 8 != 0 or Cout % 8 != 0:
                raise _abi.PpeaKernelError("transposed conv weight gradient: channels must be multiples of 8")
            # weight gradient of that conv: "input" = dy [N,Cout,Ho,Wo], "output gradient" = x [N,Cin,H,W]
            ws = torch.empty(_abi.lib.ppea_conv_wgrad_workspace_bytes(N, Cout, Cin, R, S, stride, H, W) // 4, device=dz.device,
                             dtype=_F32)
            gdt = w.dtype if w.dtype in (_BF16, _F32) else _F32
            dw = torch.empty(Cin, Cout, R, S, device=dz.device, dtype=gdt)
            call("ppea_conv_wgrad_nhwc_bf16", _raw(x), _raw(dz), ptr(dw), int(gdt == _BF16), ptr(ws), N, Ho, Wo, Cout, Cin, R, S,
                 stride, pad, 0, H, W, stream_ptr())
        return dx, dw, db, None, None, None


def conv_transpose_module(m, x):
    """nn.ConvTranspose2d `m` on the implicit-GEMM kernels (bf16 step), or None when this call is not served."""
    if not (CONV_MFMA and x.is_cuda and x.dtype == _BF16 and m.groups == 1 and tuple(m.dilation) == (1, 1)
            and m.stride[0] == m.stride[1] and m.stride[0] in (1, 2) and m.kernel_size[0] == m.kernel_size[1] == 3
            and m.padding[0] == m.padding[1] and m.output_padding[0] == m.output_padding[1]
            and x.shape[1] % 8 == 0 and m.out_channels % 8 == 0):
        return None
    return _ConvTransposeNhwc.apply(x, m.weight, m.bias, m.stride[0], m.padding[0], m.output_padding[0])


# ---------------------------------------------------------------------------------------------
# A12 / A14  dense convolutions as implicit GEMMs on the matrix cores (csrc/conv_nhwc.hip, conv_wgrad.hip):
# decoder ConvBlock / Conv3x3 (layers.py:103-135), pose ResNet-18 + PoseDecoder, reduce_conv, stem[0]
# ---------------------------------------------------------------------------------------------
CONV_ACT = {"none": 0, "relu": 1, "elu": 2, "sigmoid": 3}
CONV_MFMA = True       # dense convs of the bf16 step on this build's implicit-GEMM kernels (False: library convs)


def bf16_autocast():
    return torch.is_autocast_enabled() and torch.get_autocast_gpu_dtype() == _BF16


def conv_module(conv, x, act="none", reflect=False, out_nchw=False):
    """nn.Conv2d `conv` applied through the implicit-GEMM kernels when the bf16 step is running (x bf16, or an fp32
    image under bf16 autocast for the image-fed layers); None when this call is not served (caller uses the library)."""
    if not (CONV_MFMA and x.is_cuda and conv.groups == 1 and tuple(conv.dilation) == (1, 1)
            and conv.stride[0] == conv.stride[1] and conv.stride[0] in (1, 2)
            and conv.kernel_size[0] == conv.kernel_size[1] and conv.kernel_size[0] in (1, 3, 7)       # kernels built
            and not isinstance(conv.padding, str) and conv.padding[0] == conv.padding[1]
            and getattr(conv, "padding_mode", "zeros") == "zeros"):
        return None
    if x.dtype == _F32 and x.shape[1] < 8 and bf16_autocast():
        x = image_to_nhwc(x, 8)
    if x.dtype != _BF16 or x.shape[1] % 8 != 0:
        return None
    if reflect and (x.shape[2] < 3 or x.shape[3] < 3):        # the fold kernel of the data gradient needs a 3 x 3 interior
        return None
    return conv2d_nhwc(x, conv.weight, conv.bias, conv.stride[0], 1 if reflect else conv.padding[0], reflect, act, out_nchw)


def _pack_source(w):
    """The weight as the conv pack kernels read it: contiguous fp32 or bf16."""
    wd = w.detach()
    return wd if wd.dtype in (_F32, _BF16) and wd.is_contiguous() else wd.float().contiguous()


def _conv_packed(w, flip):
    """bf16 operand image of w [Cout,Cin,R,S] (flip: the data-gradient operand)."""
    def build(w):
        Cout, Cin, R, S = w.shape
        wd = _pack_source(w)
        buf = torch.empty(_abi.lib.ppea_conv_packed_bytes(Cout, Cin, R, S, int(flip)) // 2, dtype=_BF16, device=w.device)
        call("ppea_conv_pack_weights", ptr(wd), int(wd.dtype == _BF16), ptr(buf), Cout, Cin, R, S, int(flip), stream_ptr())
        return buf
    return _weight_image(w, ("conv", bool(flip)), build)


def _nhwc_raw(t):
    """Pointer of a channels_last (or C == 1 / 1x1 degenerate) 4-D tensor's storage."""
    return _ct.c_void_p(t.data_ptr())


def _as_nhwc(t):
    return t if t.is_contiguous(memory_format=torch.channels_last) else t.contiguous(memory_format=torch.channels_last)


# ---------------------------------------------------------------------------------------------
# decoder glue: nearest 2x upsampling + skip concatenation in one pass (channels_last)
# ---------------------------------------------------------------------------------------------
def up2cat_supported(a, b=None):
    ok = (a.is_cuda and a.dim() == 4 and a.dtype in (_F32, _BF16) and a.shape[1] % 8 == 0
          and a.is_contiguous(memory_format=torch.channels_last))
    if ok and b is not None:
        ok = (b.dtype == a.dtype and b.shape[1] % 8 == 0 and b.shape[0] == a.shape[0]
              and tuple(b.shape[2:]) == (2 * a.shape[2], 2 * a.shape[3])
              and b.is_contiguous(memory_format=torch.channels_last))
    return ok


class _Up2Cat(torch.autograd.Function):
    """cat([interpolate(a, scale_factor=2, mode="nearest"), b], 1) on channels_last tensors in ONE pass; backward
    splits the gradient and sums the upsampled part over each 2x2 block (fp32 accumulation) in one pass."""

    @staticmethod
    def forward(ctx, a, b):
        N, C1, h, w = a.shape
        C2 = 0 if b is None else b.shape[1]
        out = torch.empty(N, C1 + C2, 2 * h, 2 * w, device=a.device, dtype=a.dtype, memory_format=torch.channels_last)
        call(f"ppea_nhwc_up2cat_fwd_{_suffix(a)}", _nhwc_raw(a), None if b is None else _nhwc_raw(b), _nhwc_raw(out),
             N, 2 * h, 2 * w, C1, C2, stream_ptr())
        ctx.dims = (N, C1, C2, h, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        N, C1, C2, h, w = ctx.dims
        dout = _as_nhwc(dout)
        da = torch.empty(N, C1, h, w, device=dout.device, dtype=dout.dtype, memory_format=torch.channels_last)
        db = None if C2 == 0 else torch.empty(N, C2, 2 * h, 2 * w, device=dout.device, dtype=dout.dtype,
                                              memory_format=torch.channels_last)
        call(f"ppea_nhwc_up2cat_bwd_{_suffix(dout)}", _nhwc_raw(dout), _nhwc_raw(da), None if db is None else _nhwc_raw(db),
             N, 2 * h, 2 * w, C1, C2, stream_ptr())
        return da, db


def upsample2x_cat(a, b=None):
    return _Up2Cat.apply(a, b)


def conv_nhwc_raw(x, wp, bias, Cout, R, S, stride, pad, reflect, dil, Ho, Wo, act, out_nchw, out=None):
    """One launch of the implicit-GEMM kernel.  x: bf16, channels_last storage, logical [N,Cin,H,W].  `out`: the result's
    storage, a dense bf16 [N,Cout,Ho,Wo] tensor of the layout `out_nchw` names (default: a fresh one)."""
    N, Cin, H, W = x.shape
    if out is not None:
        fmt = torch.contiguous_format if out_nchw else torch.channels_last
        if not (out.is_cuda and out.dtype == _BF16 and tuple(out.shape) == (N, Cout, Ho, Wo) and out.is_contiguous(memory_format=fmt)):
            raise PpeaKernelError("conv_nhwc_raw: `out` must be a dense bf16 [N,Cout,Ho,Wo] tensor of the requested layout")
        y = out
    elif out_nchw:
        y = torch.empty(N, Cout, Ho, Wo, device=x.device, dtype=_BF16)
    else:
        y = torch.empty(N, Cout, Ho, Wo, device=x.device, dtype=_BF16, memory_format=torch.channels_last)
    bp, bflag = _bias_arg(bias)
    call("ppea_conv_nhwc_bf16", _nhwc_raw(x), ptr(wp), bp, bflag, _nhwc_raw(y), N, H, W, Cin, Cout, R, S, stride, pad,
         int(reflect), dil, Ho, Wo, act, int(out_nchw), stream_ptr())
    return y


WGRAD_SPLIT_RULES = ("want", "cap", "floor", "fill", "patches")


def conv_nhwc_plan(N, H, W, Cin, Cout, K, stride, pad, reflect, dil, Ho, Wo, out_nchw):
    """The kernel ppea_conv_nhwc_bf16 launches for these arguments (host only, works without a device):
    dict(NTC, BN, RPS, TR, TC) -- NTC > 0: the persistent kernel, else conv_nhwc_kernel<BN, ., ., stride, out_nchw, K, RPS>."""
    out = (_ct.c_int * 5)()
    call("ppea_conv_nhwc_plan", N, H, W, Cin, Cout, K, K, stride, pad, int(reflect), dil, Ho, Wo, int(out_nchw), out)
    return dict(zip(("NTC", "BN", "RPS", "TR", "TC"), out))


def conv_wgrad_plan(N, Cin, Cout, K, stride, Ho, Wo):
    """The plan ppea_conv_wgrad_nhwc_bf16 launches by (host only): conv_wgrad_kernel<stride, K, BM, BN>, its split over
    output patches, what set it (`split_rule`, one of WGRAD_SPLIT_RULES) and the slab reducer."""
    out = (_ct.c_int * 12)()
    call("ppea_conv_wgrad_plan", N, Cin, Cout, K, K, stride, Ho, Wo, out)
    p = dict(zip(("BM", "BN", "WK", "splits", "slabs", "rows_per_block", "rgroups", "TR", "TC", "n_patches", "split_rule",
                  "tree_reduce"), out))
    p["split_rule"] = WGRAD_SPLIT_RULES[p["split_rule"]]
    return p


PWCONV_PLAN_FIELDS = ("version", "BM", "BK", "WN", "grid_x", "grid_y", "grid_z", "partials")
PWGRAD_PLAN_FIELDS = ("step", "steps_per_image", "total_steps", "steps_per_split", "S", "tiles_m", "tiles_n")


def pwconv_plan(B, M, K, HW, transposed=False):
    """The kernel ppea_pwconv_bf16 / _stats_bf16 / _ex_bf16 / _infer_bf16 launch for these arguments under the hooks set right
    now (host only, works without a device): dict of PWCONV_PLAN_FIELDS, or None where the entry points do not serve the shape."""
    out = (_ct.c_int * 8)()
    if not try_call("ppea_pwconv_plan", B, M, K, HW, int(transposed), out):
        return None
    return dict(zip(PWCONV_PLAN_FIELDS, out))


DWCONV3X3_ARMS = ("generic", "dw3v_s1", "dw3v_s2_fwd", "dw3v_s2_bwd")
DWCONV3X3_MODES = ("forward", "data_gradient", "affine_forward")


def dwconv3x3_plan(dtype, mode, N, C, H, W, stride):
    """The kernel ppea_dwconv3x3_fwd_* / _bwd_data_* / _fwd_affine_* launch for these arguments (host only, works without a
    device): the index into DWCONV3X3_ARMS, or None where the entry points do not serve the shape.  `mode`: one of
    DWCONV3X3_MODES or its index."""
    m = DWCONV3X3_MODES.index(mode) if isinstance(mode, str) else int(mode)
    arm = _abi.lib.ppea_dwconv3x3_plan(4 if dtype == _F32 else 2, m, N, C, H, W, stride)
    if arm == -1:
        return None
    _abi.check(0 if arm >= 0 else arm, "ppea_dwconv3x3_plan")
    return arm


def pwconv_plan_sweep(B, transposed, Mstep, nM, nK, nHW):
    """pwconv_plan for one B and A mode over M = Mstep * (1..nM) x K = 32 * (1..nK) x HW = 8 * (1..nHW) (host only) ->
    (uint8 tensor [nM, nK, nHW] of packed plans: bit 0 version 2, bits 1-2 BM (32, 64, 128), bit 3 BK = 64, 255 not served;
    dict(served, partials_mismatch))."""
    out = torch.empty(nM, nK, nHW, dtype=torch.uint8)
    summary = (_ct.c_long * 2)()
    call("ppea_pwconv_plan_sweep", B, int(transposed), Mstep, nM, nK, nHW, _ct.c_void_p(out.data_ptr()), summary)
    return out, dict(served=summary[0], partials_mismatch=summary[1])


def _pwgrad_plan_dict(out):
    p = dict(zip(PWGRAD_PLAN_FIELDS, out))
    p["workspace_bytes"] = out[7] + (out[8] << 31)
    return p


def pwgrad_plan(B, M, N, HW):
    """The split ppea_pwgrad_bf16 / ppea_pwgrad_ex_bf16 launch by (host only): dict of PWGRAD_PLAN_FIELDS + workspace_bytes;
    step 0: pwgrad_kernel (64 pixels per step), 32: pwgrad2_kernel<32>.  None where they do not serve the shape."""
    out = (_ct.c_int * 9)()
    if not try_call("ppea_pwgrad_plan", B, M, N, HW, out):
        return None
    return _pwgrad_plan_dict(out)


def pwgrad_pair_plan(B, Ms, Ns, HW):
    """The same for ppea_pwgrad_ex_pair_bf16 (tiles_m / tiles_n: the tiles of problem 0 / of problem 1); None: not served."""
    out = (_ct.c_int * 9)()
    if not try_call("ppea_pwgrad_pair_plan", B, (_ct.c_int * 2)(*Ms), (_ct.c_int * 2)(*Ns), HW, out):
        return None
    return _pwgrad_plan_dict(out)


DWCONV_LK_PLAN_FIELDS = ("family", "partials", "lds_bytes", "NSEG", "WS", "BN", "BA", "band", "G", "bands", "segs",
                         "items_per_channel", "wpc", "ipw", "fast", "H", "NY", "NTX", "RS", "VEC", "gi", "ngroups", "wgpc", "cpw")
DWCONV_LK_VARIANTS = ("plain", "stats", "bn", "bias_act")


def dwconv_lk_plan(N, C, H, W, K, KS, mode=0, variant="plain"):
    """The kernel and launch geometry the MFMA depthwise entry points go by (host only, works without a device), as a dict
    of DWCONV_LK_PLAN_FIELDS.  mode 0 forward / 1 data gradient; variant one of DWCONV_LK_VARIANTS.  family 0: not served,
    1: dwconv_mfma_kernel<K, KS, mode, NSEG, BN, WS, BA>, 2: dwconv_bm_kernel<K, KS, mode, H, NY, NTX, RS, BN>."""
    out = (_ct.c_int * 24)()
    call("ppea_dwconv_lk_plan", N, C, H, W, K, KS, mode, DWCONV_LK_VARIANTS.index(variant), out)
    return dict(zip(DWCONV_LK_PLAN_FIELDS, out))


def dwconv_lk_plan_sweep(K, KS, mode, variant, Nmax, Cs, Hmax, Wmax):
    """dwconv_lk_plan over N 1..Nmax x Cs x H 1..Hmax x W 1..Wmax (host only) -> (set of the distinct plans met, each a
    dict of the fields that tell arms and paths apart, summary dict)."""
    seen = (_ct.c_ubyte * (1 << 14))()
    summary = (_ct.c_long * 4)()
    cs = (_ct.c_int * len(Cs))(*Cs)
    call("ppea_dwconv_lk_plan_sweep", K, KS, mode, DWCONV_LK_VARIANTS.index(variant), Nmax, cs, len(Cs), Hmax, Wmax, seen, summary)
    plans = []
    for key in range(1 << 14):
        if not seen[key]:
            continue
        if key & 3 == 1:
            plans.append(dict(family=1, NSEG=(2, 3, 5)[(key >> 2) & 3], WS=(key >> 4) & 1, BN=(key >> 5) & 1, BA=(key >> 6) & 1,
                              band=16 * (((key >> 7) & 3) + 1), stacked=(key >> 9) & 1, multiband=(key >> 10) & 1,
                              fast=(key >> 11) & 1, multi_item=(key >> 12) & 1))
        else:
            plans.append(dict(family=2, H=(6, 12, 24, 48)[(key >> 2) & 3], NTX=(key >> 4) & 7, BN=(key >> 7) & 1,
                              VEC=8 if (key >> 8) & 1 else 4, gi=4 * (((key >> 9) & 3) + 1), multi_wg=(key >> 11) & 1))
    return plans, dict(zip(("served", "max_lds_bytes", "bad_item_split", "not_served"), summary))


def dwconv_lk_bwd_filter_plan(N, C, H, W, K, KS):
    """dict(parts, rows_per_part, rounds, vec, lds_bytes, last_rows) of ppea_dwconv_lk_bwd_filter_bf16 (host only), or None
    where that kernel does not serve the shape."""
    out = (_ct.c_int * 6)()
    if not try_call("ppea_dwconv_lk_bwd_filter_plan", N, C, H, W, K, KS, out):
        return None
    return dict(zip(("parts", "rows_per_part", "rounds", "vec", "lds_bytes", "last_rows"), out))


def dwconv_lk_f32_plan(H, W, K):
    """Index of the CFGS_<K> tile (csrc/dwconv_lk.hip) the fp32 vector kernel runs an H x W plane on; -1: the generic kernel."""
    out = (_ct.c_int * 1)()
    call("ppea_dwconv_lk_f32_plan", H, W, K, out)
    return out[0]


def conv_supported(x, w):
    return (x.is_cuda and x.dtype == _BF16 and x.dim() == 4 and x.shape[1] % 8 == 0 and w.shape[2] <= 7
            and w.shape[3] <= 7)


_SIDE = {}


def side_stream_of(main):
    """The side stream that belongs to `main` (created on first use): the student's adapters run on it."""
    key = (main.device.index, main.cuda_stream)
    side = _SIDE.get(key)
    if side is None:
        side = _SIDE[key] = torch.cuda.Stream(main.device)
    return side


class _ConvNhwc(torch.autograd.Function):
    """y = act(conv2d(x, w, stride, pad | reflection pad) + bias) -- forward, data gradient and weight gradient on the
    implicit-GEMM kernels; bias gradient and the activation's derivative in one pass before them."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, reflect, act, out_nchw):
        x = _as_nhwc(x)
        N, Cin, H, W = x.shape
        Cout, _, R, S = w.shape
        Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
        y = conv_nhwc_raw(x, _conv_packed(w, False), None if bias is None else bias.detach().contiguous(), Cout, R, S, stride,
                          pad, reflect, 1, Ho, Wo, act, out_nchw)
        ctx.save_for_backward(x, w, y if act != 0 else None)
        ctx.cfg = (stride, pad, bool(reflect), act, bool(out_nchw), bias is not None,
                   None if bias is None else bias.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        stride, pad, reflect, act, out_nchw, has_bias, bdt = ctx.cfg
        N, Cin, H, W = x.shape
        Cout, _, R, S = w.shape
        Ho, Wo = dy.shape[2], dy.shape[3]
        db = None
        # ---- dz = dy * act'(y), channels_last bf16; bias gradient ------------------------------------------------------
        if act == 2 and not out_nchw and _nhwc_c_ok(Cout):
            dy = dy.contiguous(memory_format=torch.channels_last).to(_BF16)
            slabs = _abi.lib.ppea_nhwc_bias_elu_slabs(N * Ho * Wo, Cout)
            partial = torch.empty(slabs, Cout, device=dy.device, dtype=_F32)
            dz = torch.empty_like(dy)
            call("ppea_nhwc_bias_elu_bwd_bf16", _raw(dy), _raw(y), _raw(dz), ptr(partial), N * Ho * Wo, Cout, stream_ptr())
            if has_bias and ctx.needs_input_grad[2]:
                db = partial.sum(0).to(bdt)
        else:
            if act == 1:
                dz = dy * (y > 0)
            elif act == 2:
                dz = dy * torch.where(y > 0, torch.ones_like(y), y + 1)
            elif act == 3:
                dz = dy * (y * (1 - y))
            else:
                dz = dy
            if has_bias and ctx.needs_input_grad[2]:
                db = dz.float().sum((0, 2, 3)).to(bdt)
            dz = _as_nhwc(dz.to(_BF16))
        dx = dw = None
        if ctx.needs_input_grad[0]:
            wt = _conv_packed(w, True)                           # [R*S flipped][Cin][Cout padded to 32]
            if reflect:
                # gradient on the reflection-padded domain, then folded back (layers.py:119-135)
                dpad = conv_nhwc_raw(dz, wt, None, Cin, R, S, 1, R - 1, False, stride, Ho + R - 1, Wo + S - 1, 0, False)
                dx = torch.empty(N, Cin, H, W, device=dz.device, dtype=_BF16, memory_format=torch.channels_last)
                call("ppea_nhwc_reflect_pad1_bwd_bf16", _raw(dpad), _raw(dx), N, H, W, Cin, stream_ptr())
            else:
                dx = conv_nhwc_raw(dz, wt, None, Cin, R, S, 1, R - 1 - pad, False, stride, H, W, 0, False)
        if ctx.needs_input_grad[1]:
            if Cout % 8 != 0:
                raise _abi.PpeaKernelError("conv weight gradient: output channels must be a multiple of 8 "
                                           "(pad the layer, see conv2d_nhwc)")
            ws = torch.empty(_abi.lib.ppea_conv_wgrad_workspace_bytes(N, Cin, Cout, R, S, stride, Ho, Wo) // 4, device=dz.device,
                             dtype=_F32)
            gdt = w.dtype if w.dtype in (_BF16, _F32) else _F32
            dw = torch.empty(Cout, Cin, R, S, device=dz.device, dtype=gdt)
            call("ppea_conv_wgrad_nhwc_bf16", _raw(dz), _raw(x), ptr(dw), int(gdt == _BF16), ptr(ws), N, H, W, Cin, Cout, R, S,
                 stride, pad, int(reflect), Ho, Wo, stream_ptr())
        return dx, dw, db, None, None, None, None, None


def _image_packed(w):
    """bf16 row-packed operand image of w [Cout,Cin,K,K] for the image-fed conv kernels."""
    def build(w):
        Cout, Cin, K, _ = w.shape
        wd = _pack_source(w)
        buf = torch.empty(_abi.lib.ppea_conv_image_packed_bytes(Cout, K) // 2, dtype=_BF16, device=w.device)
        call("ppea_conv_image_pack_weights", ptr(wd), int(wd.dtype == _BF16), ptr(buf), Cout, Cin, K, stream_ptr())
        return buf
    return _weight_image(w, "image", build)


class _ConvImage(torch.autograd.Function):
    """stem[0] / pose conv1 on the row-packed image kernels: x [N,8,H,W] bf16 channels_last frames (3 / 6 real channels),
    w [Cout,Cin,K,K], stride 2.  Weight gradient only (the input is the frame)."""

    @staticmethod
    def forward(ctx, x, w, pad, out_nchw):
        N, _, H, W = x.shape
        Cout, Cin, K, _ = w.shape
        Ho, Wo = (H + 2 * pad - K) // 2 + 1, (W + 2 * pad - K) // 2 + 1
        y = torch.empty(N, Cout, Ho, Wo, device=x.device, dtype=_BF16,
                        memory_format=torch.contiguous_format if out_nchw else torch.channels_last)
        call("ppea_conv_image_bf16", _nhwc_raw(x), ptr(_image_packed(w)), _nhwc_raw(y), N, H, W, Cout, K, 2, pad, Ho, Wo,
             int(out_nchw), stream_ptr())
        ctx.save_for_backward(x, w)
        ctx.pad = pad
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None, None
        N, _, H, W = x.shape
        Cout, Cin, K, _ = w.shape
        dz = _as_nhwc(dy.to(_BF16))
        Ho, Wo = dz.shape[2], dz.shape[3]
        ws = torch.empty(_abi.lib.ppea_conv_image_wgrad_workspace_bytes(N, Cout, K, Ho, Wo) // 4, device=dz.device, dtype=_F32)
        gdt = w.dtype if w.dtype in (_BF16, _F32) else _F32
        dw = torch.empty(Cout, Cin, K, K, device=dz.device, dtype=gdt)
        call("ppea_conv_image_wgrad_bf16", _raw(dz), _raw(x), ptr(dw), int(gdt == _BF16), ptr(ws), N, H, W, Cin, Cout, K, 2,
             ctx.pad, Ho, Wo, stream_ptr())
        return None, dw, None, None


def conv2d_nhwc(x, w, bias=None, stride=1, pad=0, reflect=False, act="none", out_nchw=False):
    """Dense conv on the matrix cores.  x [N,Cin,H,W] bf16 (channels_last storage preferred), w [Cout,Cin,R,S] (bf16 or
    fp32 parameter), -> [N,Cout,Ho,Wo] bf16 channels_last (or NCHW-contiguous with out_nchw).  Layers whose output
    channel count is not a multiple of 8 (disp conv: 1, pose head: 12) run zero-padded to the next multiple."""
    Cout = w.shape[0]
    if (x.shape[1] == 8 and w.shape[1] <= 8 and stride == 2 and w.shape[2] in (3, 7) and w.shape[2] == w.shape[3]
            and bias is None and act == "none" and not reflect and Cout % 8 == 0 and not x.requires_grad):
        return _ConvImage.apply(_as_nhwc(x), w, pad, out_nchw)        # stem[0] / pose conv1: one contraction per filter row
    if w.shape[1] < x.shape[1]:                 # image-fed layers: x was zero-padded to 8 channels (image_to_nhwc)
        w = torch.cat([w, w.new_zeros(Cout, x.shape[1] - w.shape[1], *w.shape[2:])], 1)
    if Cout % 8 != 0:
        padn = 8 - Cout % 8
        w8 = torch.cat([w, w.new_zeros(padn, *w.shape[1:])], 0)
        b8 = None if bias is None else torch.cat([bias, bias.new_zeros(padn)], 0)
        y = _ConvNhwc.apply(x, w8, b8, stride, pad, reflect, CONV_ACT[act], out_nchw)
        return y[:, :Cout]
    return _ConvNhwc.apply(x, w, bias, stride, pad, reflect, CONV_ACT[act], out_nchw)


def image_to_nhwc(x, cp=8, sub=0.0, div=1.0):
    """fp32 NCHW image(s) -> bf16 channels_last with the channels zero-padded to `cp`; y = (x - sub) / div."""
    x = x.contiguous().float()
    N, C, H, W = x.shape
    y = torch.empty(N, cp, H, W, device=x.device, dtype=_BF16, memory_format=torch.channels_last)
    call("ppea_image_to_nhwc_bf16", ptr(x), _nhwc_raw(y), N, C, H, W, cp, float(sub), float(div), stream_ptr())
    return y


# ---------------------------------------------------------------------------------------------
# inference (inference.DepthPredictor): eval-mode BatchNorm as a per-channel table tab = [s; o] fp32, y = s x + o, folded
# into the launch that produces or consumes the tensor.  No autograd; None when no kernel serves the call.
# ---------------------------------------------------------------------------------------------
_UNIT_VECS = {}


def unit_vecs(C, device):
    """(zeros [C], ones [C]) fp32 on `device`, allocated once."""
    key = (C, torch.device(device))
    if key not in _UNIT_VECS:
        _UNIT_VECS[key] = (torch.zeros(C, device=device), torch.ones(C, device=device))
    return _UNIT_VECS[key]


def _as(t, dtype):
    return None if t is None else t.contiguous().to(dtype)


@torch.no_grad()
def table_affine(x, tab, act=ACT_NONE, x2=None, tab2=None, r1=None, r2=None, r2_scale=1.0):
    """act(s x + o [+ s2 x2 + o2]) (+ r1) (+ r2_scale r2), NCHW: `ppea_bn_apply_*` with mean = 0, invstd = s, gamma = 1,
    beta = o."""
    x = x.contiguous()
    N, C = x.shape[0], x.shape[1]
    zero, one = unit_vecs(C, x.device)
    st = (zero, tab[0], one, tab[1]) + ((zero, tab2[0], one, tab2[1]) if x2 is not None else (None,) * 4)
    y = torch.empty_like(x)
    call(f"ppea_bn_apply_{_suffix(x)}", ptr(x), ptr(_as(x2, x.dtype)), _ptr_array(st), None, ptr(_as(r1, x.dtype)),
         ptr(_as(r2, x.dtype)), float(r2_scale), ptr(y), int(act), N, C, x.numel() // (N * C), stream_ptr())
    return y


@torch.no_grad()
def pwconv_table(x, w, tab, act=ACT_NONE, r1=None, r2=None, r2_scale=1.0, nxt=None):
    """1x1 conv with weight w [M,K(,1,1)] + table (tab None: s = 1, o = 0) + act (+ r1) (+ r2_scale r2) in the MFMA GEMM's
    epilogue -> (y, y2 = `nxt` table applied to y as stored, or None).  None when x is not bf16 or
    `ppea_pwconv_infer_bf16` does not serve the shape."""
    if x.dtype != _BF16:
        return None
    a, _ = _pw_matrices(w)
    x = x.contiguous()
    B, K, H, W = x.shape
    M = a.shape[0]
    s, o = (None, None) if tab is None else (tab[0], tab[1])
    s2, o2 = (None, None) if nxt is None else (nxt[0], nxt[1])
    y = torch.empty(B, M, H, W, device=x.device, dtype=_BF16)
    y2 = torch.empty_like(y) if nxt is not None else None
    served = try_call("ppea_pwconv_infer_bf16", ptr(a), ptr(x), ptr(s), ptr(o), int(act), ptr(_as(r1, _BF16)),
                      ptr(_as(r2, _BF16)), float(r2_scale), ptr(s2), ptr(o2), ptr(y), ptr(y2), B, M, K, H * W, stream_ptr())
    return (y, y2) if served else None


@torch.no_grad()
def dwconv_lk_bias_act(x, w, packed, bias, relu):
    """act(DW_k(x; w) + bias), w [C,1,K,K] fp32: the MFMA kernel on `packed` (pack_dwconv_filter(w, False); bf16 x), then
    the fp32-arithmetic kernel of x's dtype on w.  None when neither serves the kernel size."""
    x = x.contiguous()
    N, C, H, W = x.shape
    y = torch.empty_like(x)
    tail = (ptr(bias), int(bool(relu)), ptr(y), N, C, H, W, w.shape[-1], stream_ptr())
    if x.dtype == _BF16 and packed is not None and try_call("ppea_dwconv_lk_fwd_bias_act_bf16p", ptr(x), ptr(packed), *tail):
        return y
    return y if try_call(f"ppea_dwconv_lk_fwd_bias_act_{_suffix(x)}", ptr(x), ptr(w, _F32), *tail) else None


@torch.no_grad()
def dwconv_lk_plain(x, w):
    """DW_k(x; w), w [C,1,K,K] fp32, on the fp32-arithmetic kernels (any odd K <= 31; no packed image involved)."""
    x = x.contiguous()
    N, C, H, W = x.shape
    y = torch.empty_like(x)
    call(f"ppea_dwconv_lk_fwd_{_suffix(x)}", ptr(x), ptr(w, _F32), None, ptr(y), None, N, C, H, W, w.shape[-1], 0, stream_ptr())
    return y


@torch.no_grad()
def dwconv3x3_affine(x, w, tab, relu, stride):
    """[relu](s DW_3(x; w) + o), pad 1, in one launch; None when `ppea_dwconv3x3_fwd_affine_*` does not serve the call."""
    x = x.contiguous()
    N, C, H, W = x.shape
    y = torch.empty(N, C, (H - 1) // stride + 1, (W - 1) // stride + 1, device=x.device, dtype=x.dtype)
    wf = w.detach().float().contiguous()
    served = try_call(f"ppea_dwconv3x3_fwd_affine_{_suffix(x)}", ptr(x), ptr(wf), ptr(tab[0]), ptr(tab[1]), int(bool(relu)),
                      ptr(y), N, C, H, W, stride, stream_ptr())
    return y if served else None


@torch.no_grad()
def nhwc_table_affine(x, ab, act=ACT_NONE, res=None):
    """act(a x + b [+ res]) on channels_last tensors (`ppea_nhwc_bn_apply_*`, ab [2,C] fp32); None when the layout or the
    channel count is not served."""
    if not (nhwc_bn_supported(x) and (res is None or res.is_contiguous(memory_format=torch.channels_last))):
        return None
    N, C, H, W = x.shape
    y = torch.empty_like(x)
    call(f"ppea_nhwc_bn_apply_{_suffix(x)}", _raw(x), _raw(res), ptr(ab), _raw(y), N * H * W, C, 1, int(act), stream_ptr())
    return y


# ---------------------------------------------------------------------------------------------
# scattered state <-> one contiguous buffer (checkpoints; csrc/state_pack.hip)
# ---------------------------------------------------------------------------------------------
class SegmentLayout:
    """Where each tensor of a list sits in the packed buffer: `offsets` (bytes, multiples of 16), `nbytes`, `dtypes`,
    `shapes`, `total` bytes.  The device table of (pointer, offset, bytes, first work unit) is built once and kept while the
    tensors' addresses are the recorded ones -- state that is only ever updated in place keeps them -- and rebuilt when any
    `data_ptr` differs at the next use."""

    def __init__(self, tensors):
        unit = int(_abi.lib.ppea_pack_unit_bytes())
        self.dtypes = [t.dtype for t in tensors]
        self.shapes = [tuple(t.shape) for t in tensors]
        self.nbytes = [t.numel() * t.element_size() for t in tensors]
        self.offsets, self.first_unit, at, units = [], [], 0, 0
        for n in self.nbytes:
            self.offsets.append(at)
            self.first_unit.append(units)
            at += (n + 15) // 16 * 16
            units += (n + unit - 1) // unit
        self.total, self.units = at, units
        self._ptrs, self._table = None, None

    def table(self, tensors):
        if len(tensors) != len(self.nbytes):
            raise PpeaKernelError(f"the layout describes {len(self.nbytes)} tensors, got {len(tensors)}")
        dev = None
        for t, n, dt in zip(tensors, self.nbytes, self.dtypes):
            if not t.is_cuda:
                raise PpeaKernelError("PPEA-Depth HIP kernels need tensors on a HIP device (no CPU fallback); got a CPU tensor")
            if not t.is_contiguous():
                raise PpeaKernelError("non-contiguous tensor passed to a HIP kernel")
            if t.numel() * t.element_size() != n or t.dtype != dt:
                raise PpeaKernelError(f"tensor of {t.numel()} x {t.dtype} where the layout has {n} bytes of {dt}")
            if dev is not None and t.device != dev:
                raise PpeaKernelError("the segments of one launch live on one device")
            dev = t.device
        ptrs = tuple(t.data_ptr() for t in tensors)
        if ptrs != self._ptrs:
            rows = [[p, o, n, u] for p, o, n, u in zip(ptrs, self.offsets, self.nbytes, self.first_unit)]
            self._table = torch.tensor(rows, dtype=torch.int64).to(dev)
            self._ptrs = ptrs
        return self._table

    def views(self, buffer):
        """The packed buffer (any device) as one tensor per segment, with the segment's dtype and shape."""
        return [buffer[o:o + n].view(dt).view(shape)
                for o, n, dt, shape in zip(self.offsets, self.nbytes, self.dtypes, self.shapes)]


@torch.no_grad()
def pack_segments(tensors, out=None, layout=None):
    """Device tensors of any dtypes -> (uint8 buffer holding their bytes back to back at 16-byte aligned offsets, layout),
    ONE launch.  `out`: a uint8 device buffer of at least `layout.total` bytes to write into (bytes past that, and the
    padding between segments, are left alone); `layout`: the one an earlier call returned for these tensors."""
    tensors = list(tensors)
    if not tensors:
        raise PpeaKernelError("pack_segments: no tensors")
    if layout is None:
        layout = SegmentLayout(tensors)
    table = layout.table(tensors)
    if out is None:
        out = torch.zeros(max(layout.total, 16), dtype=torch.uint8, device=table.device)
    if out.dtype != torch.uint8 or out.numel() < layout.total or out.device != table.device or out.data_ptr() % 16:
        raise PpeaKernelError(f"pack_segments: out must be a 16-byte aligned uint8 buffer of >= {layout.total} bytes on {table.device}")
    call("ppea_pack_segments", ptr(table), len(tensors), layout.units, ptr(out), stream_ptr())
    return out, layout


@torch.no_grad()
def unpack_segments(buffer, layout, tensors):
    """The reverse of `pack_segments`: the bytes of `buffer` written into `tensors` (in place), ONE launch."""
    tensors = list(tensors)
    table = layout.table(tensors)
    if not buffer.is_cuda:
        raise PpeaKernelError("PPEA-Depth HIP kernels need tensors on a HIP device (no CPU fallback); got a CPU tensor")
    if buffer.dtype != torch.uint8 or buffer.numel() < layout.total or buffer.device != table.device or buffer.data_ptr() % 16:
        raise PpeaKernelError(f"unpack_segments: the buffer must be 16-byte aligned uint8 of >= {layout.total} bytes on {table.device}")
    call("ppea_unpack_segments", ptr(table), len(tensors), layout.units, ptr(buffer), stream_ptr())


# ---------------------------------------------------------------------------------------------
# run monitor: one row per training step on a device ring (csrc/run_monitor.hip; the ring's owner is runlog.RunLog)
# ---------------------------------------------------------------------------------------------
MONITOR_MAX_SCALARS = 8
MONITOR_ROW_WORDS = 16


def run_monitor_scratch(device):
    """The scan's per-block partials, sized by the library for this device: fp64 [blocks * 3]."""
    return torch.zeros(int(_abi.lib.ppea_run_monitor_max_blocks()) * 3, device=device, dtype=torch.float64)


def _monitor_row_host(scalars, grads, step, grad_scale, ring, state):
    """The row of `ppea_run_monitor_f32` computed with torch in float64 on host tensors, same layout and same roundings."""
    import numpy as np
    words = ring.numpy().view(np.uint32)
    st = state.numpy()
    row = words[int(st[0]) % ring.shape[0]]
    row[:] = 0
    bad = False
    for k, s in enumerate(scalars):
        if s is None:
            continue
        bits = s.detach().reshape(1).numpy().view(np.uint32)[0]
        row[k] = bits
        row[10] |= np.uint32(1 << k)
        bad = bad or (int(bits) & 0x7f800000) == 0x7f800000
    gs = float(np.float32(grad_scale))
    total, biggest, nonfinite = 0.0, 0.0, 0
    if grads is not None and grads.numel():
        g = grads.detach().double()
        finite = torch.isfinite(g)
        nonfinite = int(g.numel() - int(finite.sum()))
        g = torch.where(finite, g, torch.zeros_like(g))
        total, biggest = float((g * g).sum()), float(g.abs().max())
    row[8:10] = np.array([gs * float(np.sqrt(total)), gs * biggest], dtype=np.float64).astype(np.float32).view(np.uint32)
    row[12:16] = np.array([int(step), nonfinite], dtype=np.int64).view(np.uint32)
    st[0] += 1
    if (bad or nonfinite > 0) and st[1] < 0:
        st[1] = int(step)


@torch.no_grad()
def run_monitor(scalars, grads, n, step, grad_scale, ring, state, scratch=None):
    """Append one row to `ring` (int32 [capacity,16]; `state` int64 [2] = rows appended, first_bad_step): up to 8 fp32
    scalars (0-dim or one-element tensors, None = absent) copied bit for bit, and of the first `n` elements of the flat fp32
    buffer `grads` (None / n = 0: none) the norm grad_scale * sqrt(sum of squares of the finite elements) accumulated in
    fp64, grad_scale * max |x| over the finite elements and the exact count of non-finite ones.  Row layout:
    include/ppea_depth.h.  On a HIP device: TWO launches on the current stream, no host read, no allocation; the scalars'
    addresses travel as kernel arguments.  Every tensor on the host: the same arithmetic with torch in float64."""
    scalars = list(scalars)
    if len(scalars) > MONITOR_MAX_SCALARS:
        raise PpeaKernelError(f"run_monitor: {len(scalars)} scalars, a row holds {MONITOR_MAX_SCALARS}")
    if ring.dtype != torch.int32 or ring.dim() != 2 or ring.shape[1] != MONITOR_ROW_WORDS or ring.shape[0] < 1 \
            or not ring.is_contiguous() or state.dtype != torch.int64 or state.numel() != 2 or not state.is_contiguous() \
            or state.device != ring.device:
        raise PpeaKernelError("run_monitor: ring is int32 [capacity,16] and state int64 [2], contiguous, on one device")
    dev = ring.device
    for k, s in enumerate(scalars):
        if s is None:
            continue
        if s.device != dev:
            raise PpeaKernelError(f"run_monitor: scalar {k} is on {s.device}, the ring on {dev}: host and device tensors "
                                  "do not mix")
        if s.dtype != torch.float32 or s.numel() != 1:
            raise PpeaKernelError(f"run_monitor: scalar {k} is {tuple(s.shape)} {s.dtype}; expected one fp32 element")
    if grads is not None:
        if grads.device != dev:
            raise PpeaKernelError(f"run_monitor: the gradient buffer is on {grads.device}, the ring on {dev}: host and "
                                  "device tensors do not mix")
        if grads.dtype != torch.float32:
            raise PpeaKernelError(f"run_monitor: the gradient buffer is {grads.dtype}; expected torch.float32")
        if not grads.is_contiguous():
            raise PpeaKernelError("run_monitor: non-contiguous gradient buffer")
        n = grads.numel() if n is None else int(n)
        if n < 0 or n > grads.numel():
            raise PpeaKernelError(f"run_monitor: n = {n} of a buffer of {grads.numel()} elements")
    else:
        n = 0
    if dev.type != "cuda":
        _monitor_row_host(scalars, None if grads is None else grads.reshape(-1)[:n], step, grad_scale, ring, state)
        return
    if n > 0 and (scratch is None or scratch.device != dev or scratch.dtype != torch.float64 or not scratch.is_contiguous()):
        raise PpeaKernelError("run_monitor: scratch is a contiguous fp64 buffer on the ring's device (run_monitor_scratch)")
    ptrs = (_ct.c_void_p * MONITOR_MAX_SCALARS)(*[None if s is None else s.data_ptr() for s in scalars])
    call("ppea_run_monitor_f32", ptrs, _ct.c_void_p(grads.data_ptr()) if n > 0 else None, n, int(step), float(grad_scale),
         ptr(scratch) if n > 0 else None, scratch.numel() // 3 if n > 0 else 0, ptr(ring), ring.shape[0], ptr(state),
         stream_ptr())
