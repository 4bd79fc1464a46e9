"""TEST INFRASTRUCTURE ONLY -- one launch of each entry point of the stencil and glue kernels (csrc/dwconv3x3.hip,
csrc/nhwc_decoder.hip, csrc/bias_act.hip, csrc/pad.hip, csrc/nhwc_pool.hip) on one row of oracle/glue_inputs.py, through the raw
ABI into NaN-filled views of guarded buffers: an element never stored is outside its bound, a store past either end changes a
guard.  GUARD elements of 2 or 4 bytes keep every view 16-byte aligned, as the kernels' vector accesses assume of the tensors
torch hands them.  tests/test_glue_arms_gpu.py holds the results to the float64 references.  Every launcher returns
(served, outputs by name, [(guarded buffer, dtype)])."""
import torch

from oracle import glue_inputs as G

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8


def to(inp, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in inp.items()}


def _out(shape, dtype, device, bufs):
    buf, t = G.guarded_u8(shape, device) if dtype == U8 else G.guarded(shape, dtype, device)
    assert t.data_ptr() % 16 == 0
    bufs.append((buf, dtype))
    return t


def untouched(outs, bufs):
    """Nothing written: every output still NaN (the index still 0xFF), every guard intact."""
    clean = all(bool((t == 0xFF).all()) if t.dtype == U8 else bool(torch.isnan(t).all()) for t in outs.values())
    return clean and all(G.guards_ok(b, dt) for b, dt in bufs)


def launch_dw(ops, c, inp, what):
    """what: fwd | bwd | aff0 | aff1 -> (served, dict(what=...), bufs)."""
    dt, dev, bufs = G.dt_of(c.dt), inp["x"].device, []
    Ho, Wo = G.out_hw(c.H, c.W, c.stride)
    ptr, st, dims = ops.ptr, ops.stream_ptr(), (c.N, c.C, c.H, c.W, c.stride)
    if what == "bwd":
        out = _out((c.N, c.C, c.H, c.W), dt, dev, bufs)
        served = ops.try_call(f"ppea_dwconv3x3_bwd_data_{c.dt}", ptr(inp["dy"]), ptr(inp["w"]), ptr(out), *dims, st)
    else:
        out = _out((c.N, c.C, Ho, Wo), dt, dev, bufs)
        if what == "fwd":
            served = ops.try_call(f"ppea_dwconv3x3_fwd_{c.dt}", ptr(inp["x"]), ptr(inp["w"]), ptr(out), *dims, st)
        else:
            served = ops.try_call(f"ppea_dwconv3x3_fwd_affine_{c.dt}", ptr(inp["x"]), ptr(inp["w"]), ptr(inp["s"]), ptr(inp["o"]),
                                  int(what == "aff1"), ptr(out), *dims, st)
    return served, {what: out}, bufs


def launch_wg(ops, c, inp, nbytes):
    """The filter gradient into a guarded dw and a guarded workspace of exactly `nbytes` -> (served, dict(dw, ws), bufs)."""
    dev, bufs = inp["x"].device, []
    dw = _out((c.C, 1, 3, 3), F32, dev, bufs)
    ws = _out((c.C, max(nbytes, 36 * c.C) // (36 * c.C), 9), F32, dev, bufs)
    served = ops.try_call(f"ppea_dwconv3x3_bwd_filter_{c.dt}", ops.ptr(inp["x"]), ops.ptr(inp["dy"]), ops.ptr(dw), ops.ptr(ws),
                          c.N, c.C, c.H, c.W, c.stride, ops.stream_ptr())
    return served, dict(dw=dw, ws=ws), bufs


def launch_pd(ops, c, inp):
    dt, dev, bufs = G.dt_of(c.dt), inp["a"].device, []
    Ho, Wo = (c.H, c.W) if c.bwd else (c.H + 2, c.W + 2)
    way = "bwd" if c.bwd else "fwd"
    if c.layout == "nhwc":
        out = _out((c.B, Ho, Wo, c.C), dt, dev, bufs)
        served = ops.try_call(f"ppea_nhwc_reflect_pad1_{way}_{c.dt}", ops.ptr(inp["a"]), ops.ptr(out), c.B, c.H, c.W, c.C, ops.stream_ptr())
    else:
        out = _out((c.B, c.C, Ho, Wo), dt, dev, bufs)
        served = ops.try_call(f"ppea_reflect_pad1_{way}_{c.dt}", ops.ptr(inp["a"]), ops.ptr(out), c.B * c.C, c.H, c.W, ops.stream_ptr())
    return served, dict(out=out), bufs


def _be_dims(c):
    return (c.N * c.HW, c.C) if c.layout == "nhwc" else (c.N, c.C, c.HW)


def _be_entry(c, way):
    return f"ppea_{'nhwc_' if c.layout == 'nhwc' else ''}bias_elu_{way}_{c.dt}"


def launch_be_fwd(ops, c, inp):
    bufs = []
    y = _out(G.be_shape(c), G.dt_of(c.dt), inp["z"].device, bufs)
    bp, bflag = ops._bias_arg(inp["bias"])
    served = ops.try_call(_be_entry(c, "fwd"), ops.ptr(inp["z"]), bp, bflag, ops.ptr(y), *_be_dims(c), ops.stream_ptr())
    return served, dict(y=y), bufs


def launch_be_bwd(ops, c, inp, y_in, partial_shape):
    """dz and the partial sums, the latter held to exactly the count the library's query gave."""
    bufs, dev = [], inp["z"].device
    dz = _out(G.be_shape(c), G.dt_of(c.dt), dev, bufs)
    partial = _out(partial_shape, F32, dev, bufs)
    served = ops.try_call(_be_entry(c, "bwd"), ops.ptr(inp["dy"]), ops.ptr(y_in), ops.ptr(dz), ops.ptr(partial), *_be_dims(c), ops.stream_ptr())
    return served, dict(dz=dz, partial=partial), bufs


def launch_uc(ops, c, inp):
    """Forward and backward -> (both served, dict(out, da [, db]), bufs)."""
    dt, dev, bufs = G.dt_of(c.dt), inp["a"].device, []
    dims, st, ptr = (c.N, c.H, c.W, c.C1, c.C2), ops.stream_ptr(), ops.ptr
    out = _out((c.N, c.H, c.W, c.C1 + c.C2), dt, dev, bufs)
    da = _out((c.N, c.H // 2, c.W // 2, c.C1), dt, dev, bufs)
    db = _out((c.N, c.H, c.W, c.C2), dt, dev, bufs) if c.C2 else None
    served = (ops.try_call(f"ppea_nhwc_up2cat_fwd_{c.dt}", ptr(inp["a"]), ptr(inp["b"]), ptr(out), *dims, st)
              and ops.try_call(f"ppea_nhwc_up2cat_bwd_{c.dt}", ptr(inp["dout"]), ptr(da), ptr(db), *dims, st))
    got = dict(out=out, da=da)
    if db is not None:
        got["db"] = db
    return served, got, bufs


def launch_mp(ops, c, inp):
    """Forward, then the backward on the index the forward stored -> (both served, dict(y, idx, dx), bufs)."""
    dt, dev, bufs = G.dt_of(c.dt), inp["x"].device, []
    Ho, Wo = G.out_hw(c.H, c.W, 2)
    dims, st, ptr = (c.N, c.H, c.W, c.C), ops.stream_ptr(), ops.ptr
    y = _out((c.N, Ho, Wo, c.C), dt, dev, bufs)
    idx = _out((c.N, Ho, Wo, c.C), U8, dev, bufs)
    dx = _out((c.N, c.H, c.W, c.C), dt, dev, bufs)
    served = (ops.try_call(f"ppea_nhwc_maxpool3x3s2_fwd_{c.dt}", ptr(inp["x"]), ptr(y), ptr(idx), *dims, st)
              and ops.try_call(f"ppea_nhwc_maxpool3x3s2_bwd_{c.dt}", ptr(inp["dy"]), ptr(idx), ptr(dx), *dims, st))
    return served, dict(y=y, idx=idx, dx=dx), bufs
