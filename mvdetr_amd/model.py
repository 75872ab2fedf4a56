"""Minimal caller of the fusion path: an MVDeTr-shaped detector whose warp and deformable attention
run on the HIP kernels.  The trunk's and the heads' convolutions are ordinary PyTorch-ROCm, as in the
reference; in inference the trunk's BatchNorm / ReLU / residual-add / max-pool passes between them run
fused on HIP kernels (ops/trunk_epilogue.py), and as the modules' own torch ops everywhere else; the stride-1 3x3
convolutions of layer1-4 that measured faster that way run as an fp32 Winograd MFMA kernel (ops/conv_winograd.py).

Mirrors multiview_detector/models/mvdetr.py:74-218 (constructor arithmetic, forward order, output
tuple) and the dilated ResNet-18 trunk of multiview_detector/models/resnet.py:33-70,120-186
(``replace_stride_with_dilation=[False, True, True]``, children()[:-2] -> stride 8, 512 channels;
parameter names follow ``base.<child index>...`` so reference checkpoints line up).  Weights are
seeded random: there is no network for the pretrained download (resnet.py:213-216).
"""
from __future__ import annotations

import threading

import torch
from torch import nn

from . import geometry
from .ops import warp_perspective
from .ops.conv_winograd import (winograd_conv3x3, winograd_conv3x3_available, winograd_conv3x3_bn_act,
                                winograd_conv3x3_bn_act_available, winograd_conv3x3_train,
                                winograd_conv3x3_train_available)
from .ops.detect import bev_detect
from .ops.peak_detect import peak_detect, PeakDetections
from .ops.ingest import ingest_frames
from .ops.trunk_epilogue import (bn_act, bn_act_half, bn_relu_maxpool, bn_relu_maxpool_half, fused_bn_act_available,
                                  fused_bn_act_half_available, fused_bn_relu_maxpool_available,
                                  fused_bn_relu_maxpool_half_available)
from .world_feat import ConvWorldFeat, DeformConvWorldFeat, DeformTransWorldFeat, TransformerWorldFeat


def _fused_bn_act(out, bn, residual=None, residual_bn=None):
    """The fused pass that takes these arguments -- bn_act for fp32 activations, bn_act_half for 16-bit ones (asked in
    that order) -- or None."""
    if fused_bn_act_available(out, bn, residual, residual_bn):
        return bn_act
    if fused_bn_act_half_available(out, bn, residual, residual_bn):
        return bn_act_half
    return None


def _conv3x3(x, conv):
    """conv(x): the fp32 Winograd kernel where it takes these arguments (inference, wide 3x3 convolutions at the trunk's
    size; under autograd its differentiable form, on the families of TRAIN_FAMILIES), torch's convolution otherwise."""
    if winograd_conv3x3_available(x, conv):
        return winograd_conv3x3(x, conv)
    if winograd_conv3x3_train_available(x, conv):
        return winograd_conv3x3_train(x, conv)
    return conv(x)


def _bn_relu(out, bn, relu):
    """relu(bn(out)) for a convolution's fresh output: one in-place HIP pass in inference, torch's ops otherwise."""
    if type(relu) is nn.ReLU:
        op = _fused_bn_act(out, bn)
        if op is not None:
            return op(out, bn, relu=True, inplace=True)
    return relu(bn(out))


def _bn_add_relu(out, bn, x, downsample, relu):
    """The tail of a residual block, relu(bn(out) + identity), where identity is the block's input x or
    downsample(x) = BatchNorm(1x1 convolution(x)).  In inference one HIP pass over ``out`` (the last convolution's
    fresh output, overwritten in place) that reads the identity branch -- the downsample convolution's raw output goes
    through its BatchNorm in the same pass; x itself is never written.  torch's ops otherwise, as in the reference."""
    if type(relu) is nn.ReLU:
        if downsample is None:
            op = _fused_bn_act(out, bn, x)
            if op is not None:
                return op(out, bn, x, relu=True, inplace=True)
        elif type(downsample) is nn.Sequential and len(downsample) == 2 and type(downsample[0]) is nn.Conv2d \
                and _fused_bn_act(out, bn) is not None:
            raw = downsample[0](x)
            op = _fused_bn_act(out, bn, raw, downsample[1])
            if op is not None:
                return op(out, bn, raw, downsample[1], relu=True, inplace=True)
            return relu(bn(out) + downsample[1](raw))
    identity = x if downsample is None else downsample(x)
    return relu(bn(out) + identity)


def _conv3x3_bn_relu(x, conv, bn, relu):
    """relu(bn(conv(x))): one Winograd launch with the epilogue in its store where that takes these arguments, the
    convolution and the pass behind it otherwise."""
    if type(relu) is nn.ReLU and winograd_conv3x3_bn_act_available(x, conv, bn):
        return winograd_conv3x3_bn_act(x, conv, bn, relu=True)
    return _bn_relu(_conv3x3(x, conv), bn, relu)


def _conv3x3_bn_add_relu(out, conv, bn, x, downsample, relu):
    """The tail of a BasicBlock, relu(bn(conv(out)) + identity), as one Winograd launch that reads the identity branch in
    its store -- x itself, or the downsample convolution's raw output (run first) through its BatchNorm; x is never
    written -- where that takes these arguments, and as _conv3x3 + _bn_add_relu otherwise."""
    if type(relu) is nn.ReLU:
        if downsample is None:
            if winograd_conv3x3_bn_act_available(out, conv, bn, x):
                return winograd_conv3x3_bn_act(out, conv, bn, x, relu=True)
        elif type(downsample) is nn.Sequential and len(downsample) == 2 and type(downsample[0]) is nn.Conv2d \
                and winograd_conv3x3_bn_act_available(out, conv, bn):
            raw = downsample[0](x)
            if winograd_conv3x3_bn_act_available(out, conv, bn, raw, downsample[1]):
                return winograd_conv3x3_bn_act(out, conv, bn, raw, downsample[1], relu=True)
            y = _conv3x3(out, conv)
            op = _fused_bn_act(y, bn, raw, downsample[1])
            if op is not None:
                return op(y, bn, raw, downsample[1], relu=True, inplace=True)
            return relu(bn(y) + downsample[1](raw))
    return _bn_add_relu(_conv3x3(out, conv), bn, x, downsample, relu)


class ResNetTrunk(nn.Sequential):
    """The trunk as the reference slices it -- conv1, bn1, relu, maxpool, layer1..4 at child indices 0..7, so parameter
    names are ``base.<index>...`` -- whose forward runs children 1-3 (BatchNorm, ReLU, MaxPool2d(3, 2, 1)) as one HIP
    pass over the stem convolution's output when that is eligible, and child by child otherwise."""

    def forward(self, x):
        mods = list(self)
        if len(mods) >= 4 and type(mods[0]) is nn.Conv2d:
            x = mods[0](x)
            if fused_bn_relu_maxpool_available(x, mods[1], mods[2], mods[3]):
                x = bn_relu_maxpool(x, mods[1])
                mods = mods[4:]
            elif fused_bn_relu_maxpool_half_available(x, mods[1], mods[2], mods[3]):
                x = bn_relu_maxpool_half(x, mods[1])
                mods = mods[4:]
            else:
                mods = mods[1:]
        for m in mods:
            x = m(x)
        return x


class BasicBlock(nn.Module):
    """3x3-3x3 residual block; only the FIRST conv is dilated (resnet.py:46-51 of the fork)."""

    def __init__(self, inplanes, planes, stride=1, downsample=None, dilation=1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, padding=dilation, dilation=dilation, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        out = _conv3x3_bn_relu(x, self.conv1, self.bn1, self.relu)
        return _conv3x3_bn_add_relu(out, self.conv2, self.bn2, x, self.downsample, self.relu)


class Bottleneck(nn.Module):
    """1x1 - 3x3 (strided / dilated) - 1x1 residual block, expansion 4 (resnet.py:72-112): the block of the
    ResNet-50 that BASELINE.json's configs[3] names.  The reference defines resnet50 (resnet.py:244) but wires only
    vgg11 / resnet18 into the detector (mvdetr.py:97-107)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, dilation=1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, padding=dilation, dilation=dilation, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        out = _bn_relu(self.conv1(x), self.bn1, self.relu)
        out = _conv3x3_bn_relu(out, self.conv2, self.bn2, self.relu)
        return _bn_add_relu(self.conv3(out), self.bn3, x, self.downsample, self.relu)


def resnet_trunk(depth=18, replace_stride_with_dilation=(False, True, True), in_channels=3) -> nn.Sequential:
    """conv1, bn1, relu, maxpool, layer1..4 as one Sequential (the reference slices
    list(resnet18(...).children())[:-2], mvdetr.py:103-105).  depth 18: BasicBlock x [2,2,2,2], 512 channels out;
    depth 50: Bottleneck x [3,4,6,3], 2048 channels out (resnet.py:226-250)."""
    block, counts = {18: (BasicBlock, (2, 2, 2, 2)), 50: (Bottleneck, (3, 4, 6, 3))}[depth]
    exp = getattr(block, "expansion", 1)
    state = {"inplanes": 64, "dilation": 1}

    def make_layer(planes, blocks, stride=1, dilate=False):
        prev = state["dilation"]
        if dilate:
            state["dilation"] *= stride
            stride = 1
        down = None
        if stride != 1 or state["inplanes"] != planes * exp:
            down = nn.Sequential(nn.Conv2d(state["inplanes"], planes * exp, 1, stride, bias=False), nn.BatchNorm2d(planes * exp))
        layers = [block(state["inplanes"], planes, stride, down, prev)]
        state["inplanes"] = planes * exp
        layers += [block(planes * exp, planes, dilation=state["dilation"]) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    trunk = ResNetTrunk(
        nn.Conv2d(in_channels, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
        nn.MaxPool2d(3, 2, 1),
        make_layer(64, counts[0]), make_layer(128, counts[1], 2, replace_stride_with_dilation[0]),
        make_layer(256, counts[2], 2, replace_stride_with_dilation[1]), make_layer(512, counts[3], 2, replace_stride_with_dilation[2]))
    for m in trunk.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
    return trunk


def resnet18_trunk(replace_stride_with_dilation=(False, True, True), in_channels=3) -> nn.Sequential:
    return resnet_trunk(18, replace_stride_with_dilation, in_channels)


def output_head(in_dim, feat_dim, out_dim):
    # mvdetr.py:24-30
    if feat_dim:
        return nn.Sequential(nn.Conv2d(in_dim, feat_dim, 3, padding=1), nn.ReLU(), nn.Conv2d(feat_dim, out_dim, 1))
    return nn.Sequential(nn.Conv2d(in_dim, out_dim, 1))


class _ProjUpload:
    """Uploads of the per-frame projection matrices for one (device, thread): a ring of three pinned staging buffers (the
    host only waits for the upload issued three frames ago, not for the previous frame's -- which queues behind that
    frame's kernels), and the last upload is handed out again while the matrices do not change (no augmentation: the
    same device tensor every frame, so that consumers keyed on it -- the warp gradient's plan -- see it unchanged)."""
    RING = 3

    def __init__(self):
        self.bufs, self.events, self.next = [], [], 0
        self.last_host, self.last_dev = None, None

    def upload(self, proj, dev):
        if self.last_host is not None and self.last_dev is not None and self.last_dev.device == dev \
                and self.last_host.shape == proj.shape and torch.equal(self.last_host, proj):
            return self.last_dev
        if not self.bufs or self.bufs[0].shape != proj.shape:
            self.bufs = [torch.empty_like(proj).pin_memory() for _ in range(self.RING)]
            self.events = [None] * self.RING
            self.next = 0
        i = self.next
        self.next = (i + 1) % self.RING
        if self.events[i] is not None:
            self.events[i].synchronize()                                  # that buffer's previous upload has left it
        self.bufs[i].copy_(proj)
        out = self.bufs[i].to(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self.events[i] = ev
        self.last_host, self.last_dev = proj.clone(), out
        return out


class MVDeTr(nn.Module):
    def __init__(self, geom: geometry.SceneGeometry, Ks, Rts, arch="resnet18", z=0, world_feat_arch="deform_trans",
                 bottleneck_dim=None, outfeat_dim=0, dropout=0.5, channels_last=True):
        super().__init__()
        self.geom = geom
        self.Rimg_shape, self.Rworld_shape = geom.Rimg_shape, geom.Rworld_shape
        self.img_reduce, self.num_cam = geom.img_reduce, geom.num_cam
        self.channels_last = channels_last
        self.compute_dtype = None                                          # set by to_inference(): float16 / bfloat16
        bottleneck_dim = geom.feat_channels if bottleneck_dim is None else bottleneck_dim
        # image pixel -> reduced world grid, fp64 (mvdetr.py:82-95)
        self.register_buffer("proj_mats", torch.from_numpy(geometry.build_proj_mats(geom, Ks, Rts, z)), persistent=False)
        # host copy for the per-frame composition: the buffer above follows .to(device) (it is part of the reference's
        # attribute set, mvdetr.py:95), and reading it back every forward would be a full-stream sync per frame
        self._proj_mats_host, self._proj_host_src, self._proj_host_version = None, None, None
        self._transient = {}
        if arch not in ("resnet18", "resnet50"):
            raise ValueError("trunks: resnet18 (the reference's default, mvdetr.py:102-105) or resnet50 (BASELINE configs[3]; "
                             "resnet.py:244); vgg11 is not provided")
        self.base = resnet_trunk(int(arch[6:]))
        base_dim = 512 if arch == "resnet18" else 2048
        if bottleneck_dim:
            self.bottleneck = nn.Sequential(nn.Conv2d(base_dim, bottleneck_dim, 1), nn.Dropout2d(dropout))
            base_dim = bottleneck_dim
        else:
            self.bottleneck = nn.Identity()
        self.img_heatmap = output_head(base_dim, outfeat_dim, 1)
        self.img_offset = output_head(base_dim, outfeat_dim, 2)
        self.img_wh = output_head(base_dim, outfeat_dim, 2)
        self.world_feat_arch = world_feat_arch
        if world_feat_arch == "deform_trans":
            n_points = 4
            ref = geometry.create_reference_map(geom, Ks, Rts, n_points).repeat([geom.num_cam, 1, 1, 1])
            self.world_feat = DeformTransWorldFeat(geom.num_cam, geom.Rworld_shape, base_dim, hidden_dim=base_dim,
                                                   n_points=n_points, stride=2, reference_points=ref)
        elif world_feat_arch == "conv":
            self.world_feat = ConvWorldFeat(geom.num_cam, geom.Rworld_shape, base_dim, hidden_dim=base_dim)
        elif world_feat_arch == "deform_conv":
            # the world heads take base_dim channels (mvdetr.py:139-140): the reference's default hidden_dim=128 is base_dim
            self.world_feat = DeformConvWorldFeat(geom.num_cam, geom.Rworld_shape, base_dim, hidden_dim=base_dim)
        elif world_feat_arch == "trans":
            # as for deform_conv: the world heads take base_dim channels, and the aggregator views its encoder output with
            # the input's channel count (trans_world_feat.py:66)
            self.world_feat = TransformerWorldFeat(geom.num_cam, geom.Rworld_shape, base_dim, hidden_dim=base_dim)
        else:
            raise ValueError("world_feat_arch must be 'deform_trans', 'conv', 'deform_conv' or 'trans'")
        self.world_heatmap = output_head(base_dim, outfeat_dim, 1)
        self.world_offset = output_head(base_dim, outfeat_dim, 2)
        # init (mvdetr.py:142-148)
        self.img_heatmap[-1].bias.data.fill_(-2.19)
        self.world_heatmap[-1].bias.data.fill_(-2.19)
        for head in (self.img_offset, self.img_wh, self.world_offset):
            for m in head.modules():
                if isinstance(m, nn.Conv2d) and m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def frame_proj_mats(self, M, device=None):
        """[B*N,3,3] fp32 reduced world grid <- feature pixel, composed on the host in fp32 exactly like
        mvdetr.py:155-161 (M is the dataloader's augmentation matrix and lives on the CPU there).  With ``device`` the
        result is uploaded from a pinned staging buffer with a non-blocking copy: nothing in a frame waits for the GPU,
        so the host can queue frame k+1 behind frame k (the reference composes on the CPU and does a pageable
        ``.to(device)`` every forward, mvdetr.py:194)."""
        pm = self.proj_mats
        # (the source tensor itself is held and compared with `is`: an id() alone can be reused by a later tensor)
        if pm is not self._proj_host_src or pm._version != self._proj_host_version:
            self._proj_mats_host = pm.detach().cpu().clone()              # one sync, after .to(device) / in-place edits
            self._proj_host_src, self._proj_host_version = pm, pm._version
        proj = geometry.compose_frame_proj_mats(self._proj_mats_host, M.cpu(), self.img_reduce)
        if device is None or torch.device(device).type == "cpu":
            return proj
        dev = torch.device(device)
        t = self._transient.setdefault((dev.type, dev.index, threading.get_ident()), _ProjUpload())
        return t.upload(proj, dev)

    # the pinned staging buffers / events / cached uploads are per (device, thread) run-time state, not part of the model:
    # they are not pickled, deep-copied or shared between DataParallel replicas' threads
    def __getstate__(self):
        d = dict(self.__dict__)
        d["_transient"] = {}
        d["_proj_mats_host"], d["_proj_host_src"], d["_proj_host_version"] = None, None, None
        return d

    def __deepcopy__(self, memo):
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__getstate__().items():
            new.__dict__[k] = copy.deepcopy(v, memo)
        return new

    def to_inference(self, dtype):
        """Convert the model for 16-bit INFERENCE (``dtype`` = torch.float16 or torch.bfloat16; forward only, under
        ``no_grad``) and return it, in eval mode.  What ``nn.Module.half()`` would get wrong is left alone:

          * convolution, linear, LayerNorm and embedding parameters and the position embedding (the ``conv`` aggregator's
            coordinate map likewise) are cast to ``dtype``: the trunk's and the heads' convolutions and the encoder's GEMMs
            run on the matrix units in 16 bits;
          * BatchNorm2d parameters and running statistics stay float32 (torch's batch norm takes 16-bit activations with
            float32 statistics);
          * ``proj_mats`` (float64) and the encoder's ``reference_points`` / ``reference_shared`` (float32) are not touched,
            bit for bit: a [0, 1] coordinate in bfloat16 is +-0.7 px on a 180-wide map.  ``frame_proj_mats`` stays float32.

        The warp (fp32 matrices, fp64 source positions), the fused deformable attention (fp32 reference points, softmax and
        locations) and the add + LayerNorm tails (fp32 statistics) run their 16-bit-storage HIP kernels, each rounding once
        on the way out; so do the trunk's BatchNorm / ReLU / residual-add / max-pool epilogues (ops/trunk_epilogue.py:
        16-bit activations, the float32 BatchNorm vectors kept above; ``bn(x) + identity`` is not rounded in between).
        ``forward`` then returns 16-bit head maps; ``detect`` upcasts the two world maps for the detection extraction.
        Served for all four world features.  ``trans`` (its encoder's attention core is the 16-bit MFMA kernel of
        csrc/attention_half.hip) and ``deform_conv`` (its deformable convolutions are dc_fwd_mfma_half of
        csrc/deform_conv_half.hip) have no 16-bit host path: the model must be on a CUDA device when it is converted.
        Training, ``torch.autocast`` and the backward are not part of it."""
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("to_inference: dtype must be torch.float16 or torch.bfloat16")
        if self.world_feat_arch == "deform_conv" and not all(p.is_cuda for p in self.parameters()):
            raise NotImplementedError("to_inference: the 'deform_conv' world feature's 16-bit deformable convolution is "
                                      "GPU-only (there is no 16-bit host path): move the model to a CUDA device first, "
                                      "then convert it")
        if self.world_feat_arch == "trans" and not all(p.is_cuda for p in self.parameters()):
            raise NotImplementedError("to_inference: the 'trans' world feature's 16-bit attention is GPU-only (there is no "
                                      "16-bit host path): move the model to a CUDA device first, then convert it")
        self.eval()
        for m in self.modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                continue
            for p in m._parameters.values():
                if p is not None and p.is_floating_point():
                    p.data = p.data.to(dtype)
            if hasattr(m, "cache_fused_projection"):
                m._fused_cache = None                                      # (a cached permuted weight has the old dtype)
            if hasattr(m, "_half_weight_cache"):
                m._half_weight_cache = None                                # (DeformConv2d's permuted 16-bit weight likewise)
        for name in ("pos_embedding", "coord_map"):
            if name in self.world_feat._buffers and self.world_feat._buffers[name] is not None:
                self.world_feat._buffers[name] = self.world_feat._buffers[name].to(dtype)
        self.compute_dtype = dtype
        return self

    def ingest(self, frames, M=None):
        """Decoded camera frames, uint8 ``[B, N, Hs, Ws, 3]`` (or ``[N, Hs, Ws, 3]``: one frame), -> the ``imgs`` that ``forward``,
        ``detect`` and the training step take, ``[B, N, 3, H, W]`` at the geometry's ``input_img_shape``: the dataset's ToTensor,
        Normalize and Resize (frameDataset.py:66-67,199-206) -- and, with ``M [B, N, 3, 3]``, its augmentation warp of the image
        (image_utils.py:43; the SAME ``M`` then goes to ``forward``) -- as one HIP pass (ops/ingest.py).  The result has the model's
        compute dtype and, with ``channels_last``, is a view of a ``[B N, 3, H, W]`` channels-last tensor: ``features`` then copies
        nothing."""
        if frames.dim() == 4:
            frames = frames.unsqueeze(0)
        return ingest_frames(frames, M, out_hw=self.geom.input_img_shape, dtype=self.compute_dtype or torch.float32,
                             channels_last=self.channels_last)

    def detect_frames(self, frames, M=None, **detect_kw):
        """``detect(self.ingest(frames, M), M, **detect_kw)``; without ``M`` the frames are not augmented (identity matrices)."""
        if frames.dim() == 4:
            frames = frames.unsqueeze(0)
        imgs = self.ingest(frames, M)
        if M is None:
            M = torch.eye(3).repeat(frames.shape[0], frames.shape[1], 1, 1)
        return self.detect(imgs, M, **detect_kw)

    def features(self, imgs):
        B, N, C, H, W = imgs.shape
        if self.compute_dtype is not None:
            imgs = imgs.to(self.compute_dtype)
        x = imgs.reshape(B * N, C, H, W)
        if self.channels_last:
            x = x.contiguous(memory_format=torch.channels_last)
        return self.bottleneck(self.base(x))

    def forward(self, imgs, M, visualize=False):
        B, N = imgs.shape[:2]
        proj = self.frame_proj_mats(M, imgs.device)
        feat = self.features(imgs)                                         # [B*N, C, h, w]
        imgs_heatmap, imgs_offset, imgs_wh = self.img_heatmap(feat), self.img_offset(feat), self.img_wh(feat)
        H, W = self.Rworld_shape
        C = feat.shape[1]
        nhwc = self.channels_last and self.world_feat_arch in ("deform_trans", "deform_conv")
        world = warp_perspective(feat, proj, (H, W), channels_last_out=nhwc)
        world = world.view(B, N, H, W, C) if nhwc else world.view(B, N, C, H, W)
        world = self.world_feat(world)
        return (self.world_heatmap(world), self.world_offset(world)), (imgs_heatmap, imgs_offset, imgs_wh)

    def detect(self, imgs, M, **detect_kw):
        """Inference down to ground-plane detections: ``forward`` under ``no_grad``, then the fused decode + threshold + distance
        NMS (ops/detect.py, the tail of the reference's test loop, trainer.py:121-135) on the world head's outputs where they
        live.  ``detect_kw`` are ``bev_detect``'s (cls_thres, dist_thres, top_k, indexing, max_det); ``world_reduce`` defaults to
        the geometry's.  Returns ``bev_detect``'s result object, all on the device: nothing here waits for the GPU.  The forward
        goes through ``__call__``, so a forward hook on the model sees the very maps the detections come from."""
        with torch.no_grad():
            (world_heatmap, world_offset), _ = self(imgs, M)
        detect_kw.setdefault("world_reduce", self.geom.world_reduce)
        if self.compute_dtype is not None:
            # 16-bit inference: the extraction is float32 / float64 (thresholds, positions); two small maps are upcast
            world_heatmap, world_offset = world_heatmap.float(), world_offset.float()
        return bev_detect(world_heatmap, world_offset, **detect_kw)

    def detect_views(self, imgs, M, *, view_top_k=100, view_cls_thres=None, **detect_kw):
        """``detect`` plus the per-view detections of the same forward: ``(Detections, PeakDetections)``.  The first is exactly
        what ``detect(imgs, M, **detect_kw)`` returns.  The second is the fused peak + top-K decode (ops/peak_detect.py, the
        reference's ``ctdet_decode`` of trainer.py:173) of the three image-plane maps with ``scale = img_reduce``, so its boxes
        are pixels of the dataset's ``img_shape`` frame and its points the foot points (frameDataset.py:207-208); every tensor's
        leading dimension is viewed as ``[B, N, ...]`` and ``count`` as ``[B, N]``.  One ``self(imgs, M)`` under ``no_grad``
        serves both, through ``__call__`` (hooks see the maps); nothing waits for the GPU.  A ``to_inference`` model's five
        maps are upcast to float32 first."""
        B, N = imgs.shape[:2]
        with torch.no_grad():
            (world_heatmap, world_offset), (imgs_heatmap, imgs_offset, imgs_wh) = self(imgs, M)
        detect_kw.setdefault("world_reduce", self.geom.world_reduce)
        if self.compute_dtype is not None:
            world_heatmap, world_offset = world_heatmap.float(), world_offset.float()
            imgs_heatmap, imgs_offset, imgs_wh = imgs_heatmap.float(), imgs_offset.float(), imgs_wh.float()
        det = bev_detect(world_heatmap, world_offset, **detect_kw)
        views = peak_detect(imgs_heatmap, imgs_offset, imgs_wh, top_k=view_top_k, cls_thres=view_cls_thres,
                            scale=self.geom.img_reduce)
        return det, PeakDetections(*[t.view(B, N, *t.shape[1:]) for t in views])

    def hot_path(self, feat, proj):
        """warp + shadow transformer only (the path BASELINE.json's north_star names), for timing."""
        H, W = self.Rworld_shape
        N = self.num_cam
        B = feat.shape[0] // N
        nhwc = self.channels_last and self.world_feat_arch in ("deform_trans", "deform_conv")
        world = warp_perspective(feat, proj, (H, W), channels_last_out=nhwc)
        world = world.view(B, N, H, W, -1) if nhwc else world.view(B, N, -1, H, W)
        return self.world_feat(world)


def build_model(config="wildtrack", seed=0, world_feat_arch="deform_trans", **kw) -> MVDeTr:
    geom = geometry.GEOMETRIES[config]
    Ks, Rts = geometry.synthetic_rig(geom, seed=seed)
    torch.manual_seed(seed)
    return MVDeTr(geom, Ks, Rts, world_feat_arch=world_feat_arch, **kw)
