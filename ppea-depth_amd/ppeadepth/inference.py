"""Inference path: `DepthPredictor` walks a (live, possibly training-mode) `RepDepth` and launches the eval-mode schedule
itself, with every eval BatchNorm folded into a per-channel table.

In eval mode BatchNorm is y = s * x + o with s = gamma / sqrt(running_var + eps), o = beta - running_mean * s, known before
the launch.  What folds where (reference: networks/replknet_adapter.py:182-326, 511-542):

  * 1x1 conv + BN (+ ReLU / GELU) (+ residual + gamma * adapter) (+ the NEXT block's first BN as a second output):
    the epilogue of the MFMA GEMM (`ppea_pwconv_infer_bf16`).  The table is applied to the fp32 accumulator, so the
    predictor shares the training model's bf16 weight matrices: no second copy of the frozen parameters.
  * large-kernel pair BN(DW_k) + BN(DW_5) + ReLU: ONE k x k depthwise launch with the merged filter
    s_big W_k + pad(s_small W_5) (held by the predictor, packed for the MFMA depthwise kernel), bias o_big + o_small and the
    ReLU in its epilogue (`ppea_dwconv_lk_fwd_bias_act_*`).
  * depthwise 3x3 + BN + ReLU: one launch (`ppea_dwconv3x3_fwd_affine_*`).
  * stem[0] / InputAdapter convs + BN (+ act): conv kernel + one `ppea_bn_apply_*` launch.
  * stand-alone BNs (first block's prelkb_bn, `stages[s].norm`): one `ppea_bn_apply_*` launch with the constant table.
  * pose ResNet-18: `ppea_nhwc_bn_apply_*` with the (a, b) table built from the running statistics.

The predictor never replaces or deletes a module or parameter and never flips `model.training`.  Sub-modules WITHOUT
BatchNorm, dropout or DropPath (adapters, depth decoders, pose decoder, reduce_conv) compute the same function in both
modes and are called as they are.  `device="cpu"` runs the same schedule and the same tables with torch ops.
"""
import contextlib
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._abi import PpeaKernelError
from .layers import pose_chain
from .ops import ACT_GELU, ACT_NONE, ACT_RELU


def _act(x, act):
    return F.relu(x) if act == ACT_RELU else (F.gelu(x) if act == ACT_GELU else x)


def bn_table(bn):
    """(s, o) fp32 of an eval-mode BatchNorm: y = s * x + o."""
    s = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    return torch.stack([s, bn.bias.detach().float() - bn.running_mean.detach().float() * s])


def merged_lk(lk):
    """ReparamLargeKernelConv in eval mode as ONE k x k depthwise filter + bias (rka.py:250-261), from tables."""
    tb, wb = bn_table(lk.lkb_origin.bn), lk.lkb_origin.conv.weight.detach().float()
    w, bias = wb * tb[0].view(-1, 1, 1, 1), tb[1]
    if hasattr(lk, "small_conv"):
        ts, ws = bn_table(lk.small_conv.bn), lk.small_conv.conv.weight.detach().float()
        p = (wb.shape[-1] - ws.shape[-1]) // 2
        w = w + F.pad(ws * ts[0].view(-1, 1, 1, 1), [p] * 4)
        bias = bias + ts[1]
    return w.contiguous(), torch.stack([torch.ones_like(bias), bias])


def cost_volume_cpu(cur, look, poses, K, inv_K, bins, eps=1e-7):
    """torch composite of `ops.cost_volume` / `ops.cost_volume_multi` (replk_matching_adapter.py:261-340): raw cost [B,D,h,w].
    look [B,C,h,w] with poses [B,4,4], or F lookup frames as look [B,F,C,h,w] with poses [B,F,4,4]: the masked differences of
    the frames whose pose is not zeroed are summed in frame order and divided by the number of frames that contributed."""
    if look.dim() == 4:
        look, poses = look[:, None], poses[:, None]
    B, C, h, w = cur.shape
    D = bins.shape[0]
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(h * w)], 0)
    inner = torch.zeros(h, w)
    inner[2:-2, 2:-2] = 1.0
    out = []
    for b in range(B):
        cost, counts = torch.zeros(D, h, w), torch.zeros(D, h, w)
        for f in range(look.shape[1]):
            if float(poses[b, f].sum()) == 0.0:
                continue
            rays = inv_K[b, :3, :3] @ pix
            pts = torch.cat([bins.view(D, 1, 1) * rays[None], torch.ones(D, 1, h * w)], 1)
            cam = (K[b] @ poses[b, f])[:3][None] @ pts
            xy = cam[:, :2] / (cam[:, 2:3] + eps)
            gx = ((xy[:, 0] / (w - 1)) - 0.5) * 2
            gy = ((xy[:, 1] / (h - 1)) - 0.5) * 2
            grid = torch.stack([gx, gy], -1).reshape(D, h, w, 2)
            warped = F.grid_sample(look[b, f][None].expand(D, C, h, w), grid, mode="bilinear", padding_mode="zeros",
                                   align_corners=True)
            xv, yv = (grid[..., 0] / 2 + 0.5) * (w - 1), (grid[..., 1] / 2 + 0.5) * (h - 1)
            edge = ((xv >= 2.0) & (xv <= w - 2) & (yv >= 2.0) & (yv <= h - 2)).float()
            diff = (warped - cur[b:b + 1]).abs().mean(1) * (edge * inner)
            cost = cost + diff
            counts = counts + (diff > 0).float()
        out.append(cost / (counts + 1e-7))
    return torch.stack(out)


def cost_volume_reduce_cpu(raw, bins):
    """torch composite of `ops.cost_volume_reduce`: (masked cost, confidence, argmin, lowest-cost 1/depth)."""
    D = raw.shape[1]
    missing = (raw == 0).float()
    filled = raw * (1 - missing) + raw.max(1, keepdim=True)[0] * missing
    conf = (((filled * (1 - missing)) > 0).sum(1) == D).float()
    viz = torch.where(filled == 0, torch.full_like(filled, 100.0), filled)
    idx = torch.min(viz, 1)[1]
    return filled * conf.unsqueeze(1), conf, idx, 1.0 / bins[idx]


class DepthPredictor:
    def __init__(self, model, opt, amp_dtype=torch.bfloat16, device=None):
        self.model = getattr(model, "module", model)
        self.opt = opt
        mdev = next(self.model.parameters()).device
        self.device = torch.device(mdev if device is None else device)
        self.cpu = self.device.type == "cpu"
        if self.cpu:
            amp_dtype = None
            if mdev.type != "cpu":
                raise PpeaKernelError("a device='cpu' predictor needs the model on the CPU")
        elif mdev != self.device:
            raise PpeaKernelError(f"model on {mdev}, predictor asked for {self.device}")
        if amp_dtype not in (None, torch.bfloat16):
            raise PpeaKernelError(f"amp_dtype {amp_dtype} is not served (bf16 or None = fp32)")
        self.amp_dtype = amp_dtype
        self.bf16 = amp_dtype == torch.bfloat16
        # the lookup frames are the model's; an `opt` that describes another set is an inconsistency, not a request
        self.lookup_ids = [int(f) for f in self.model.matching_ids[1:]]
        asked = ([1] if getattr(opt, "use_future_frame", False) else []) + [
            -k for k in range(1, 1 + getattr(opt, "num_matching_frames", 1))]
        if asked != self.lookup_ids:
            raise PpeaKernelError(f"opt describes lookup frames {asked}, the model was built with {self.lookup_ids}")
        if not 1 <= len(self.lookup_ids) <= ops.CV_MAX_FRAMES:
            raise PpeaKernelError(f"the cost volume serves 1 .. {ops.CV_MAX_FRAMES} lookup frames, the model has "
                                  f"{len(self.lookup_ids)}")
        from .networks import replknet_adapter as rka
        self._rka = rka
        for enc in (self.model.encoder.replk, self.model.mono_encoder):
            for m in enc.modules():
                if isinstance(m, rka.ReparamLargeKernelConv):
                    if not hasattr(m, "lkb_origin"):
                        raise PpeaKernelError("structurally re-parameterised encoders are not served: build the predictor "
                                              "from the training form")
                    if not isinstance(m.lkb_origin.conv, rka.LargeKernelDW):
                        raise PpeaKernelError("large-kernel branch is not a depthwise k x k conv with k > 5")
        self.tab, self.lk, self.pose_ab = {}, {}, {}
        self._graphs = {}
        self._streams = weakref.WeakSet()
        self.refresh()

    # ---- tables ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def refresh(self):
        """Rebuild every table and merged depthwise filter from the model's CURRENT weights and running statistics, in
        place where the storage exists (a captured graph keeps reading the same buffers)."""
        from .batchnorm import BatchNorm2d
        rka = self._rka

        def put(store, key, val):
            old = store.get(key)
            if old is not None and old.shape == val.shape:
                old.copy_(val)
            else:
                store[key] = val.clone()

        for enc in (self.model.encoder.replk, self.model.mono_encoder):
            for m in enc.modules():
                if isinstance(m, (BatchNorm2d, nn.BatchNorm2d)):
                    put(self.tab, id(m), bn_table(m))
                elif isinstance(m, rka.ReparamLargeKernelConv):
                    w, tb = merged_lk(m)
                    e = self.lk.setdefault(id(m), {})
                    put(e, "w", w)
                    put(e, "tab", tb)
                    if self.bf16:         # packed in place: a captured graph keeps reading the same buffer
                        e["packed"] = (ops.pack_dwconv_filter(e["w"], False, out=e.get("packed"))
                                       if ops.dwconv_lk_packed_supported(w.shape[-1]) else None)
        for m in self.model.pose_encoder.modules():
            if isinstance(m, nn.BatchNorm2d):
                put(self.pose_ab, id(m), bn_table(m))
        for s in list(self._streams):     # features and poses computed under the old weights are never matched
            s.reset()

    # ---- primitives -----------------------------------------------------------------------------------------------
    def affine(self, x, tab, act=ACT_NONE, x2=None, tab2=None, r1=None, r2=None, r2_scale=1.0):
        """act(s x + o [+ s2 x2 + o2]) (+ r1) (+ r2_scale r2), per-channel tables, NCHW."""
        if self.cpu:
            y = x * tab[0].view(1, -1, 1, 1) + tab[1].view(1, -1, 1, 1)
            if x2 is not None:
                y = y + (x2 * tab2[0].view(1, -1, 1, 1) + tab2[1].view(1, -1, 1, 1))
            y = _act(y, act)
            if r1 is not None:
                y = y + r1
            return y if r2 is None else y + r2_scale * r2
        return ops.table_affine(x, tab, act, x2, tab2, r1, r2, r2_scale)

    def pw(self, x, conv, tab, act=ACT_NONE, r1=None, r2=None, r2_scale=1.0, nxt=None):
        """1x1 conv + table (+ act, residual, adapter add) -> (y, nxt table applied to y or None)."""
        w = conv.weight
        if self.bf16 and x.shape[1] % 32 == 0 and (x.shape[2] * x.shape[3]) % 8 == 0:      # (bf16 x: the op checks)
            out = ops.pwconv_table(x, w, tab, act, r1, r2, r2_scale, nxt)
            if out is not None:
                return out
        z = F.conv2d(x, w) if self.cpu else ops.conv2d_f32(x, w.detach())
        y = self.affine(z, tab, act, r1=r1, r2=r2, r2_scale=r2_scale)
        return y, (None if nxt is None else self.affine(y, nxt))

    def dw_lk(self, x, lk):
        """relu(BN(DW_k(x)) + BN(DW_5(x))) as one merged depthwise conv + bias + ReLU."""
        e = self.lk[id(lk)]
        w = e["w"]
        if self.cpu:
            return F.relu(F.conv2d(x, w, e["tab"][1], 1, w.shape[-1] // 2, 1, w.shape[0]))
        y = ops.dwconv_lk_bias_act(x, w, e.get("packed"), e["tab"][1], True)   # bias + ReLU in the kernel's epilogue
        if y is not None:
            return y
        # kernel sizes without a tuned tile: the one-thread-per-output kernel, then bias + ReLU as a table launch
        return self.affine(ops.dwconv_lk_plain(x, w), e["tab"], ACT_RELU)

    def conv_bn(self, x, seq, act):
        """ConvBNAct with a dense or depthwise 3x3 conv (stem[0], stem[1], stem[3], transitions[.][1])."""
        conv, tab = seq.conv, self.tab[id(seq.bn)]
        if self.cpu:
            return self.affine(F.conv2d(x, conv.weight, None, conv.stride, conv.padding, 1, conv.groups), tab, act)
        rka = self._rka
        if isinstance(conv, rka.SmallDW):
            y = ops.dwconv3x3_affine(x, conv.weight, tab, act == ACT_RELU, conv.stride[0]) if act != ACT_GELU else None
            if y is not None:
                return y
            z = ops.dwconv3x3(x, conv.weight, conv.stride[0])
        elif conv.groups == 1:
            z = ops.conv_module(conv, x, out_nchw=True) if isinstance(conv, rka.ImageConv) else None
            if z is None:
                z = ops.conv2d_f32(x if x.dtype != torch.float32 or not self.bf16 else x.to(torch.bfloat16),
                                   conv.weight.detach(), None, conv.stride[0], conv.padding[0])
        else:
            raise PpeaKernelError(f"no inference kernel for conv {conv}")
        return self.affine(z, tab, act)

    def dense(self, x, conv):
        """Dense conv with bias (InputAdapter) on this build's kernels."""
        if self.cpu:
            return F.conv2d(x, conv.weight, conv.bias, conv.stride, conv.padding)
        return ops.conv2d_f32(x, conv.weight.detach(), conv.bias, conv.stride[0], conv.padding[0])

    # ---- RepLKNet trunk -------------------------------------------------------------------------------------------
    def _stem(self, net, img):
        x = self.conv_bn(img, net.stem[0], ACT_RELU)
        adpt = None
        if net.input_adpt:
            ia = net.input_adapter
            h = self.affine(self.dense(x, ia.D_fc1), self.tab[id(ia.bn1)], ACT_GELU)
            adpt = self.affine(self.dense(h, ia.D_fc2), self.tab[id(ia.bn2)])
        x = self.conv_bn(x, net.stem[1], ACT_RELU)
        x, _ = self.pw(x, net.stem[2].conv, self.tab[id(net.stem[2].bn)], ACT_RELU)
        x = self.conv_bn(x, net.stem[3], ACT_RELU)
        return x if adpt is None else x + adpt

    def _stage(self, net, s, x):
        rka = self._rka
        blocks = net.stages[s].blocks
        pre = None
        for i, blk in enumerate(blocks):
            if pre is None:
                pre = self.affine(x, self.tab[id(blk.pre_bn)])
            nxt = self.tab[id(blocks[i + 1].pre_bn)] if i + 1 < len(blocks) else None
            if isinstance(blk, rka.RepLKBlock):
                adpt = blk.adapter(pre) if blk.test_id >= 0 else None
                t, _ = self.pw(pre, blk.pw1.conv, self.tab[id(blk.pw1.bn)], ACT_RELU)
                t = self.dw_lk(t, blk.large_kernel)
            else:
                adpt = blk.mlp_adapter(pre) if blk.test_id >= 0 else None
                t, _ = self.pw(pre, blk.pw1.conv, self.tab[id(blk.pw1.bn)], ACT_GELU)
            x, pre = self.pw(t, blk.pw2.conv, self.tab[id(blk.pw2.bn)], ACT_NONE, r1=x, r2=adpt, r2_scale=float(blk.gamma),
                             nxt=nxt)
        return x

    def _norm(self, net, s, x):
        n = net.stages[s].norm
        return x if isinstance(n, nn.Identity) else self.affine(x, self.tab[id(n)])

    def _transition(self, net, s, x):
        tr = net.transitions[s]
        x, _ = self.pw(x, tr[0].conv, self.tab[id(tr[0].bn)], ACT_RELU)
        x = self.conv_bn(x, tr[1], ACT_RELU)
        if net.trans_adpt:
            x = x + net.trans_adpt[s](x)
        return x

    def _rest(self, net, x, feats, first):
        for s in range(first, net.num_stages):
            x = self._stage(net, s, x)
            if s in net.out_indices:
                feats.append(self._norm(net, s, x))
            if s < net.num_stages - 1:
                x = self._transition(net, s, x)
        return feats

    # ---- pose network ---------------------------------------------------------------------------------------------
    def _pose_bn(self, x, bn, act, res=None):
        ab = self.pose_ab[id(bn)]
        if self.cpu:
            y = x * ab[0].view(1, -1, 1, 1) + ab[1].view(1, -1, 1, 1)
            return _act(y if res is None else y + res, act)
        y = ops.nhwc_table_affine(x, ab, act, res)
        if y is not None:
            return y
        one = ops.unit_vecs(x.shape[1], x.device)[1]
        return self.affine(x, ab, act, x2=res, tab2=None if res is None else torch.stack([one, one * 0]))

    def _pose_features(self, pair):
        from .networks import resnet_encoder as rn
        e = self.model.pose_encoder.encoder
        if self.cpu:
            conv = lambda c, x: c(x)                                   # noqa: E731
            pool = lambda x: F.max_pool2d(x, 3, 2, 1)                  # noqa: E731
            x = (pair - 0.45) / 0.225
        else:
            conv, pool = rn._conv, (lambda x: rn._maxpool(e.maxpool, x))
            x = ops.image_to_nhwc(pair, 8, 0.45, 0.225) if self.bf16 else (pair - 0.45) / 0.225
        x = pool(self._pose_bn(conv(e.conv1, x), e.bn1, ACT_RELU))
        for layer in (e.layer1, e.layer2, e.layer3, e.layer4):
            for blk in layer:
                idt = x if blk.downsample is None else self._pose_bn(conv(blk.downsample[0], x), blk.downsample[1], ACT_NONE)
                out = self._pose_bn(conv(blk.conv1, x), blk.bn1, ACT_RELU)
                x = self._pose_bn(conv(blk.conv2, out), blk.bn2, ACT_RELU, idt)
        return x

    def _poses(self, color0, looks, keep=None):
        """Relative poses 0 -> f of the lookup frames, [B,F,4,4] in `lookup_ids` order: the pairs (f, f + 1), inverted, for
        f < 0 and (f - 1, f) for f > 0 through the pose network as one F * B batch, then chained (repdepth.py:471-500).
        keep [B,F]: zero = that lookup frame is missing, its pose and every pose chained behind it are exact zeros."""
        B, ids = color0.shape[0], self.lookup_ids
        frames = {0: color0, **{f: looks[:, j] for j, f in enumerate(ids)}}
        pairs = [torch.cat([frames[f], frames[f + 1]] if f < 0 else [frames[f - 1], frames[f]], 1) for f in ids]
        x = self._pose_features(pairs[0] if len(pairs) == 1 else torch.cat(pairs, 0))
        axisangle, translation = self.model.pose([[x]])
        # (+1,) -1, -2, ...: the neighbour towards frame 0 comes first; one launch on the device (ops.pose_chain)
        return pose_chain([(axisangle[j * B:(j + 1) * B, 0], translation[j * B:(j + 1) * B, 0]) for j in range(len(ids))],
                          [(j, f < 0, -1 if f in (-1, 1) else ids.index(f + 1 if f < 0 else f - 1)) for j, f in enumerate(ids)],
                          keep)

    # ---- public ---------------------------------------------------------------------------------------------------
    def _ctx(self):
        return torch.autocast("cuda", dtype=self.amp_dtype) if self.bf16 else contextlib.nullcontext()

    @torch.no_grad()
    def _mono(self, color):
        with self._ctx():
            net = self.model.mono_encoder
            feats = self._rest(net, self._stem(net, color), [], 0)
            return self.model.mono_depth(feats)[("disp", 0)].float()

    @torch.no_grad()
    def _multi(self, color0, looks, K2, inv_K2, min_bin, max_bin, keep=None):
        """looks [B,F,3,H,W] in `lookup_ids` order -> (disp, lowest_cost, poses [B,F,4,4])."""
        with self._ctx():
            enc = self.model.encoder
            net = enc.replk
            B, Fr = looks.shape[:2]
            pose = self._poses(color0, looks, keep)
            mn = torch.as_tensor(min_bin, dtype=torch.float32, device=self.device).reshape(())
            mx = torch.as_tensor(max_bin, dtype=torch.float32, device=self.device).reshape(())
            bins = enc.compute_depth_bins(mn, mx, self.device)
            # the current and the lookup frames share stem + stage 0 (eval BatchNorm is per sample): one (1 + F) B batch
            x = self._stage(net, 0, self._stem(net, torch.cat([color0, looks.reshape(B * Fr, *looks.shape[2:])], 0)))
            feat0, look = self._norm(net, 0, x[:B]), x[B:].reshape(B, Fr, *x.shape[1:])
            if self.cpu:
                raw = cost_volume_cpu(feat0, look, pose, K2.float(), inv_K2.float(), bins)
            else:
                raw = ops.cost_volume_multi(feat0.contiguous(), look.contiguous(), pose, K2, inv_K2, bins)
            disp, lowest = self._after_sweep(feat0, raw, bins)
            return disp, lowest, pose

    def _after_sweep(self, feat0, raw, bins):
        """Raw cost [B,D,h,w] -> reduce, reduce_conv, stages 1 .. 3, decoder -> (disp, lowest_cost)."""
        enc = self.model.encoder
        net = enc.replk
        if self.cpu:
            cost, _conf, _idx, lowest = cost_volume_reduce_cpu(raw, bins)
            xr = enc.reduce_conv(torch.cat([feat0, cost], 1))
        else:
            cost, _conf, _idx, lowest = ops.cost_volume_reduce(raw, bins)
            cat = torch.cat([feat0, cost.to(feat0.dtype)], 1)
            xr = ops.conv_module(enc.reduce_conv[0], cat, "relu", out_nchw=True)
            if xr is None:
                xr = F.relu(enc.reduce_conv[0](cat))
        feats = self._rest(net, self._transition(net, 0, xr), [feat0], 1)
        return self.model.depth(feats)[("disp", 0)].float(), lowest

    def predict_mono(self, color):
        """Teacher: color [B,3,H,W] in [0,1] -> disparity [B,1,H,W] fp32."""
        g = self._graphs.get(("mono", tuple(color.shape)))
        if g is None:
            return self._mono(color.to(self.device))
        g["in"][0].copy_(color)
        g["graph"].replay()
        return g["out"].clone()

    def predict(self, color0, lookups, K2, inv_K2, min_bin, max_bin, keep=None):
        """Pose network -> cost volume -> multi-frame encoder -> decoder (as `Trainer.predict_disps`).
        lookups: [B,3,H,W] for a model with one lookup frame, or [B,F,3,H,W] in `model.matching_ids[1:]` order.
        keep: [B,F] (None: all present), zero = that lookup frame of that item is missing, the reference's rule for a missing
        image (repdepth.py:502-505): its relative pose and every pose chained behind it are exact zeros, the plane sweep skips
        it, and whatever image sits in the slot does not reach the result.  A call with `keep` runs eagerly: the captured
        graph is the call without it.
        -> dict(disp [B,1,H,W], lowest_cost [B,h/4,w/4], pose [B,4,4] resp. [B,F,4,4]: the relative poses 0 -> frame)."""
        single = lookups.dim() == 4
        looks = lookups[:, None] if single else lookups
        if looks.shape[1] != len(self.lookup_ids):
            raise PpeaKernelError(f"{looks.shape[1]} lookup frame(s) given, the model matches against {self.lookup_ids}")
        if keep is not None and tuple(keep.shape) != tuple(looks.shape[:2]):
            raise PpeaKernelError(f"keep {tuple(keep.shape)} for lookups {tuple(looks.shape[:2])}")
        g = self._graphs.get(("multi", tuple(color0.shape))) if keep is None else None
        if g is None:
            d = self.device
            out = self._multi(color0.to(d), looks.to(d), K2.to(d), inv_K2.to(d), min_bin, max_bin,
                              None if keep is None else keep.to(d))
        else:
            mn = torch.as_tensor(min_bin, dtype=torch.float32).reshape(())
            mx = torch.as_tensor(max_bin, dtype=torch.float32).reshape(())
            for dst, src in zip(g["in"], (color0, looks, K2, inv_K2, mn, mx)):
                dst.copy_(src)
            g["graph"].replay()
            out = tuple(t.clone() for t in g["out"])
        return {"disp": out[0], "lowest_cost": out[1], "pose": out[2][:, 0] if single else out[2]}

    def capture(self, B, mono=True, multi=True):
        """torch.cuda.graph over static buffers for batch B at (opt.height, opt.width); predict* then replay."""
        if self.cpu:
            raise PpeaKernelError("capture needs a HIP device")
        H, W, d = self.opt.height, self.opt.width, self.device
        img = lambda: torch.rand(B, 3, H, W, device=d)                  # noqa: E731
        eye = torch.eye(4, device=d).repeat(B, 1, 1)
        jobs = []
        if mono:
            jobs.append(("mono", [img()], lambda i: self._mono(i[0])))
        if multi:
            looks = torch.rand(B, len(self.lookup_ids), 3, H, W, device=d)
            ins = [img(), looks, eye.clone(), eye.clone(), torch.tensor(0.1, device=d), torch.tensor(10.0, device=d)]
            jobs.append(("multi", ins, lambda i: self._multi(*i)))
        for name, ins, fn in jobs:
            side = torch.cuda.Stream(d)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):                                      # warm-up: caches, lazy kernel attributes
                    fn(ins)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = fn(ins)
            self._graphs[(name, (B, 3, H, W))] = {"graph": graph, "in": ins, "out": out}
        return self

    def stream(self, B):
        """State for B parallel cameras at (opt.height, opt.width): see `DepthStream`."""
        return DepthStream(self, B)

    # ---- export: calls of their own, after predict* (they may be captured after it) ---------------------------------
    def render(self, x, size=None, **kw):
        """A colour picture of a predicted plane x [B,1,h,w] / [B,h,w] (`disp`, `lowest_cost`) at `size` (None: its own):
        `vis.colorize_device` on the current stream -> uint8 [B,H,W,3], or (flat, table) for B different sizes."""
        from . import vis
        return vis.colorize_device(x, size, **kw)

    @torch.no_grad()
    def depth(self, disp, sizes, scale=1.0, lo=1e-3, hi=80.0, mode="disp", dtype=torch.float32, out=None, min_depth=None,
              max_depth=None):
        """Metric depth at the frames' own sizes from the network's disparity `disp` [B,1,h,w]: the disparity is scaled with
        `layers.disp_to_depth(disp, opt.min_depth, opt.max_depth)` (min_depth / max_depth: other ends, e.g. `Trainer.val`'s
        1e-3 and 80) and handed to `ops.disp_export` (there: sizes, scale, clamp, mode, dtype, out and what is returned).
        A device="cpu" predictor computes the same in numpy (`evaluate.export_depth`)."""
        from .layers import disp_to_depth
        scaled, _ = disp_to_depth(disp.float(), self.opt.min_depth if min_depth is None else min_depth,
                                  self.opt.max_depth if max_depth is None else max_depth)
        if not self.cpu:
            return ops.disp_export(scaled.contiguous(), sizes, scale, lo, hi, mode, dtype, out)
        import numpy as np
        from .evaluate import export_depth
        planes = ops._planes(scaled, "depth").numpy()
        B = planes.shape[0]
        hw = ops.target_sizes(sizes, B)
        sc = scale.tolist() if torch.is_tensor(scale) else [scale] * B
        np_dtype = np.uint16 if dtype == torch.uint16 else np.float32
        return ops.host_export([export_depth(planes[b], hw[b], sc[b], lo, hi, mode, np_dtype) for b in range(B)], hw, out)


    @torch.no_grad()
    def points(self, disp, sizes, inv_K, color=None, color_offsets=None, pose=None, scale=1.0, lo=1e-3, hi=80.0, stride=1,
               edge=0.0, mode="disp", capacity=None, out=None, min_depth=None, max_depth=None):
        """3D points at the frames' own sizes from the network's disparity `disp` [B,1,h,w]: the disparity is scaled as in
        `depth` (`layers.disp_to_depth`) and handed to `ops.point_cloud` (there: sizes, scale, lo / hi, stride, edge, mode,
        capacity, out and the `ops.PointCloud` that is returned).  inv_K [B,4,4] at each frame's OWN size (`full_inv_K`);
        pose [B,4,4] camera-to-world or None (the camera frame); color: the frames' uint8 HWC bytes in one buffer
        (color_offsets [B] int64 byte offsets, None: back to back) or fp32 [B,3,H,W] in [0,1].  A call of its own on the
        current stream: it can be captured after a `predict*` or a `push`.  A device="cpu" predictor computes the same in
        numpy (`evaluate.export_points`)."""
        from .layers import disp_to_depth
        scaled, _ = disp_to_depth(disp.float(), self.opt.min_depth if min_depth is None else min_depth,
                                  self.opt.max_depth if max_depth is None else max_depth)
        if not self.cpu:
            return ops.point_cloud(scaled.contiguous(), sizes, inv_K, pose, color, color_offsets, scale, lo, hi, stride, edge,
                                   mode, capacity, out)
        import numpy as np
        from .evaluate import export_points
        planes = ops._planes(scaled, "points").numpy()
        B = planes.shape[0]
        hw = ops.target_sizes(sizes, B)
        rows, _ = ops.target_rows(hw)
        sc = scale.tolist() if torch.is_tensor(scale) else [scale] * B
        parts = []
        for b, (H, W) in enumerate(hw):
            col = None
            if color is not None and color.dtype == torch.uint8:
                off = rows[b][0] * 3 if color_offsets is None else int(color_offsets[b])
                col = color.reshape(-1)[off:off + H * W * 3].view(H, W, 3).numpy()
            elif color is not None:
                col = color[b].float().numpy()
            parts.append(export_points(planes[b], (H, W), inv_K[b].numpy(), col, None if pose is None else pose[b].numpy(),
                                       sc[b], lo, hi, stride, edge, mode, rows[b][0]))
        if out is None:
            out = ops.new_point_cloud(ops.candidate_count(hw, int(stride)) if capacity is None else int(capacity), B, "cpu",
                                      color is not None)
        cap = out.xyz.shape[0]
        start, dropped = out.cursor.tolist()
        total = sum(len(x[2]) for x in parts)
        fit = min(total, cap - start)
        out.xyz[start:start + fit] = torch.from_numpy(np.concatenate([x[0] for x in parts])[:fit])
        out.index[start:start + fit] = torch.from_numpy(np.concatenate([x[2] for x in parts])[:fit])
        if color is not None:
            out.rgb[start:start + fit] = torch.from_numpy(np.concatenate([x[1] for x in parts])[:fit])
        out.cursor[0], out.cursor[1] = start + fit, dropped + total - fit
        out.counts.copy_(torch.tensor([len(x[2]) for x in parts]))
        return out

    def full_inv_K(self, K_norm, sizes):
        """The loaders' normalised intrinsics (3x3 or 4x4, one matrix or B of them: kitti_dataset.py:26-29, row 0 in units of
        the width, row 1 of the height) -> [B,4,4] fp32 inverse intrinsics at each frame's own size `sizes` ((H, W) or B
        pairs), on the predictor's device: what `points` takes.  The inverse is taken in float64 on the host and rounded
        once."""
        import numpy as np
        K = np.asarray(K_norm.cpu() if torch.is_tensor(K_norm) else K_norm, dtype=np.float64)
        if K.ndim not in (2, 3) or K.shape[-2:] not in ((3, 3), (4, 4)):
            raise PpeaKernelError(f"K_norm {K.shape}: 3x3 or 4x4 intrinsics, one matrix or a batch")
        single = len(sizes) == 2 and not hasattr(sizes[0], "__len__")
        B = K.shape[0] if K.ndim == 3 else 1 if single else len(sizes)
        hw = ops.target_sizes(sizes, B)
        inv = np.empty((B, 4, 4), dtype=np.float32)
        for b, (H, W) in enumerate(hw):
            full = np.eye(4)
            k = K[b] if K.ndim == 3 else K
            full[:k.shape[0], :k.shape[1]] = k
            full[0] *= W
            full[1] *= H
            inv[b] = np.linalg.inv(full)
        return torch.from_numpy(inv).to(self.device)


class StreamMap:
    """One fused point cloud of a `DepthStream`: the points of every pushed frame, at the network's size, in the frame of each
    camera's first frame since its reset, appended to ONE shared `ops.PointCloud` of `capacity` points.

    `world` [B,4,4] fp32 is the camera-to-world matrix of each camera's newest frame, identity at the start.  `add` multiplies
    it from the right with the push's `pose[:, 0]` (the transform 0 -> -1: X_{t-1} = T X_t, so X_world = W_{t-1} T X_t) where
    `present[:, 0]`, and sets it to the identity where the camera has just been reset.  It is a plain fp32 product chain with
    no re-orthonormalisation: after n frames element ij is within n * 1e-6 * max(1, max_i sum_j |W_ij|) of the float64
    product of the same fp32 poses (4 products and 3 sums of at most one ulp of the absolute-value sum per step).  Loop
    closure, voxel fusion and scale alignment between clips are not done here."""

    def __init__(self, stream, capacity, stride=4, edge=0.1, lo=1e-3, hi=80.0, scale=1.0):
        self.s = stream
        self.kw = dict(stride=stride, edge=edge, lo=lo, hi=hi, scale=scale)
        d = stream.p.device
        self.world = torch.eye(4, device=d).repeat(stream.B, 1, 1).contiguous()
        self._cloud = ops.new_point_cloud(int(capacity), stream.B, d, True)

    @torch.no_grad()
    def add(self, out, color, inv_K):
        """out: what `push` returned for `color` [B,3,H,W]; inv_K [B,4,4] at the network's size (full resolution, not the
        matching scale).  Two kernels' worth of launches on the current stream, nothing read on the host: capturable."""
        s = self.s
        if s.p.cpu:
            W, P = self.world.clone(), out["pose"][:, 0].float()
            new = ((W[:, :, 0:1] * P[:, 0:1] + W[:, :, 1:2] * P[:, 1:2]) + W[:, :, 2:3] * P[:, 2:3]) + W[:, :, 3:4] * P[:, 3:4]
            self.world.copy_(torch.where(out["present"][:, 0].bool()[:, None, None], new, torch.eye(4).expand_as(new)))
        else:
            ops.pose_accumulate(self.world, out["pose"], out["present"])
        s.p.points(out["disp"], (s.H, s.W), inv_K, color=color, pose=self.world, out=self._cloud, **self.kw)
        return self

    def cloud(self):
        """The shared `ops.PointCloud` (`.trim()` reads its fill once)."""
        return self._cloud

    def clear(self):
        """Empties the buffer and puts every camera's `world` back to the identity."""
        self._cloud.clear()
        self.world.copy_(torch.eye(4, device=self.world.device).expand_as(self.world))
        return self


class DepthStream:
    """Video streaming on a `DepthPredictor`: `push` takes the NEXT frame of each of B cameras and matches it against the last
    F frames, whose stage-0 features, pose pairs and images it kept from the earlier pushes -- stem + stage 0 run on B items
    instead of (1 + F) B, the pose trunk on one pair batch instead of F.

    State (on the predictor's device; a replayed push reads no host value):
      ring       the un-normalised stage-0 output x of the last F frames, [F,B,C,h,w] fp32, or for bf16 features the plane
                 sweep's channel-pair dwords [F,B,C/2,h,w] (the reference matches `stages[0].norm(x)` of the current frame
                 against the RAW x of the lookups, replk_matching_adapter.py:357-369, 433-445);
      pose_ring  the pose decoder's raw (axisangle, translation) of the pairs (t-k-1, t-k), [F,B,2,3] fp32;
      prev       the previous frame [B,3,H,W], for the one new pair (t-1, t);
      state      int32 [1 + B]: the head slot, then per item the frames seen since its reset, clamped at F.
    Lookup j (frame t-1-j) is ring slot (head - 1 - j) mod F, pair j is pose slot (head - j) mod F.  After a reset fewer than F
    earlier frames exist: a missing lookup frame has an exact-zero pose and is skipped by the sweep (`predict`'s `keep`), and
    with none present the cost is the all-skipped volume.  `present [B,F]` says which lookups existed."""

    def __init__(self, predictor, B):
        p = self.p = predictor
        self.F = len(p.lookup_ids)
        if p.lookup_ids != [-k for k in range(1, self.F + 1)]:
            raise PpeaKernelError(f"a stream matches against the past frames -1 .. -F; the model's lookup frames are "
                                  f"{p.lookup_ids} (a future frame means a frame of latency: not served)")
        if int(B) < 1:
            raise PpeaKernelError(f"a stream needs B >= 1 cameras, got {B}")
        self.B, self.H, self.W = int(B), p.opt.height, p.opt.width
        d = p.device
        self.state = torch.zeros(1 + self.B, device=d, dtype=torch.int32)
        self.prev = torch.zeros(self.B, 3, self.H, self.W, device=d)
        self.pose_ring = torch.zeros(self.F, self.B, 2, 3, device=d)
        self.ring = None                  # allocated by the first push, from stage 0's output
        self._graph = None
        p._streams.add(self)

    def reset(self, mask=None):
        """All cameras (mask [B] bool: only those) start a new clip: their next frame has no lookup frame."""
        if mask is None:
            self.state.zero_()
        else:
            if tuple(mask.shape) != (self.B,):
                raise PpeaKernelError(f"reset: mask {tuple(mask.shape)} for {self.B} cameras")
            self.state[1:].masked_fill_(mask.to(self.state.device, torch.bool), 0)
        return self

    def _host_chain(self, aa, tr):
        """The host-side ring with the torch composites: (poses [B,F,4,4], present [B,F], lookups [B,F,C,h,w])."""
        Fr, head = self.F, int(self.state[0])
        self.pose_ring[head, :, 0], self.pose_ring[head, :, 1] = aa.reshape(-1, 3).float(), tr.reshape(-1, 3).float()
        present = self.state[1:, None] > torch.arange(Fr)[None]
        slots = [self.pose_ring[(head - j) % Fr] for j in range(Fr)]
        pose = pose_chain([(sl[:, None, 0], sl[:, None, 1]) for sl in slots], [(j, True, j - 1) for j in range(Fr)],
                          present.float())
        look = torch.stack([self.ring[(head - 1 - j) % Fr] for j in range(Fr)], 1)
        return pose, present, look

    @torch.no_grad()
    def _step(self, color, K2, inv_K2, mn, mx):
        p, Fr = self.p, self.F
        with p._ctx():
            enc = p.model.encoder
            net = enc.replk
            x = p._stage(net, 0, p._stem(net, color))
            feat0 = p._norm(net, 0, x)
            axisangle, translation = p.model.pose([[p._pose_features(torch.cat([self.prev, color], 1))]])
            aa, tr = axisangle[:, 0], translation[:, 0]
            bins = enc.compute_depth_bins(mn, mx, p.device)
            pairs = p.bf16 and ops.CV_BF16 and x.dtype == torch.bfloat16 and x.shape[1] % 2 == 0
            if self.ring is None:
                B, C, h, w = x.shape
                self.ring = (torch.zeros(Fr, B, C // 2, h, w, device=p.device, dtype=torch.int32) if pairs else
                             torch.zeros(Fr, B, C, h, w, device=p.device))
            if p.cpu:
                pose, present, look = self._host_chain(aa, tr)
                raw = cost_volume_cpu(feat0, look, pose, K2.float(), inv_K2.float(), bins)
            else:
                pose, present = ops.pose_chain_ring(self.pose_ring, self.state, (aa, tr))
                # the chain wrote zeros exactly where seen[b] <= j, which the sweep tests itself: no zero-pose flags
                raw = ops.cost_volume_ring(feat0.contiguous() if pairs else feat0.float().contiguous(), self.ring, self.state,
                                           pose, K2, inv_K2, bins, zero_pose_skip=False)
            disp, lowest = p._after_sweep(feat0, raw, bins)
            # the sweep has read the slot that holds frame t - F: it is overwritten now
            if p.cpu:
                head = int(self.state[0])
                self.ring[head] = x.float()
                self.state[0] = (head + 1) % Fr
                self.state[1:] = (self.state[1:] + 1).clamp(max=Fr)
            else:
                ops.ring_store(x.contiguous() if pairs else x.float().contiguous(), self.ring, self.state)
                ops.ring_advance(self.state, Fr)
            self.prev.copy_(color)
            return disp, lowest, pose, present

    def push(self, color, K2, inv_K2, min_bin, max_bin):
        """color [B,3,H,W] in [0,1]: the next frame of each camera; K2, inv_K2 [B,4,4] at the matching scale.
        -> dict(disp [B,1,H,W] fp32, lowest_cost [B,h/4,w/4], pose [B,F,4,4] relative poses 0 -> -1 .. -F (zeros where the
        frame is missing), present [B,F] bool)."""
        if tuple(color.shape) != (self.B, 3, self.H, self.W):
            raise PpeaKernelError(f"push: color {tuple(color.shape)}, the stream was opened for {(self.B, 3, self.H, self.W)}")
        d = self.p.device
        g = self._graph
        if g is None:
            mn = torch.as_tensor(min_bin, dtype=torch.float32, device=d).reshape(())
            mx = torch.as_tensor(max_bin, dtype=torch.float32, device=d).reshape(())
            out = self._step(color.to(d), K2.to(d), inv_K2.to(d), mn, mx)
        else:
            mn = torch.as_tensor(min_bin, dtype=torch.float32).reshape(())
            mx = torch.as_tensor(max_bin, dtype=torch.float32).reshape(())
            for dst, src in zip(g["in"], (color, K2, inv_K2, mn, mx)):
                dst.copy_(src)
            g["graph"].replay()
            out = tuple(t.clone() for t in g["out"])
        return {"disp": out[0], "lowest_cost": out[1], "pose": out[2], "present": out[3]}

    def render(self, out, /, what="disp", size=None, **kw):
        """A colour picture of what a push returned: out (positional) = `push`'s dict, what "disp" or "lowest_cost"; `size`
        and the keywords as `vis.colorize_device` (range, percentile, cmap, and its own `out=`: the picture's buffer).  A
        call of its own on the current stream."""
        if what not in ("disp", "lowest_cost"):
            raise PpeaKernelError(f"render: what {what!r}, expected 'disp' or 'lowest_cost'")
        return self.p.render(out[what], size, **kw)

    def map(self, capacity, stride=4, edge=0.1, lo=1e-3, hi=80.0, scale=1.0):
        """A `StreamMap` of `capacity` points fed by this stream's pushes: `m.add(push(...), color, inv_K)`."""
        return StreamMap(self, capacity, stride, edge, lo, hi, scale)

    def capture(self):
        """One torch.cuda.graph over static buffers for a whole push, state update included (single stream, no parallel
        branches); every later push replays it.  The stream is reset: the warm-up frames are not part of any clip."""
        p = self.p
        if p.cpu:
            raise PpeaKernelError("capture needs a HIP device")
        d = p.device
        eye = torch.eye(4, device=d).repeat(self.B, 1, 1)
        ins = [torch.rand(self.B, 3, self.H, self.W, device=d), eye.clone(), eye.clone(), torch.tensor(0.1, device=d),
               torch.tensor(10.0, device=d)]
        side = torch.cuda.Stream(d)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):                                      # warm-up: caches, lazy kernel attributes, the ring
                self._step(*ins)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = self._step(*ins)
        self._graph = {"graph": graph, "in": ins, "out": out}
        return self.reset()
