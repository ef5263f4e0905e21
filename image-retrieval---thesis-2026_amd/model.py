"""Embedding models with the reference's forward() contract (model.py of the reference).

Contract kept (reference model.py:50-84): ``DenseNet121(pretrained, embedding_dim, num_labels)``,
``forward(x: float[B,3,H,W]) -> float[B,D]`` with unit-norm rows (eps 1e-12), a dict with
``"embedding"``/``"logits"`` when ``num_labels`` is set, attributes ``densenet121`` (Sequential
whose child ``0`` is the feature stack and whose child ``avgpool`` is the pooling), ``fc``,
``classification_head``; state-dict keys ``densenet121.0.conv0.weight``,
``densenet121.0.denseblock1.denselayer1.norm1.weight``, ..., ``densenet121.0.norm5.*``,
``fc.*`` load unchanged.

The backbone is restated here from the published DenseNet-121 definition (Huang et al.;
torchvision is NOT a dependency and is absent offline): conv0 7x7/2 (3->64), BN, ReLU,
max-pool 3x3/2, dense blocks of (6, 12, 24, 16) layers [BN-ReLU-conv1x1(->128)-BN-ReLU-
conv3x3(->32)], transitions [BN-ReLU-conv1x1(halve)-avgpool 2x2], norm5.  6 953 856
feature parameters, final map [B,1024,H/32,W/32].

MI355X path (CUDA tensors, eval mode):
  * stem conv0+norm0+relu0+pool0 -> one HIP kernel (libmirx ``mirx_stem_conv7_bn_relu_pool``)
  * dense blocks: convolutions run under PyTorch-ROCm (MIOpen / rocBLAS, fp32); each block owns
    ONE preallocated feature buffer (no O(L^2) torch.cat re-copies); norm1+relu1 is one HIP pass
    over the buffer's channel prefix (``mirx_bn_relu_nchw``); norm2 is folded into conv1
  * transitions: norm+relu+avgpool in one HIP pass (``mirx_bn_relu_avgpool2``), then the 1x1
    conv on the pooled map (conv and average pool commute)
  * norm5+relu+global-average-pool+flatten+F.normalize -> one HIP kernel
    (``mirx_bn_relu_gap_l2norm``), or GAP only when an ``fc`` follows.
``pretrained=True`` would need a download in the reference (model.py:53); here it raises
unless a local state dict is given via ``weights=``.
"""
import ctypes
import dataclasses
import math
import operator
import weakref
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

IMAGENET_MEAN = (0.485, 0.456, 0.406)          # reference test.py:1309-1310
IMAGENET_STD = (0.229, 0.224, 0.225)
BLOCK_CONFIG = (6, 12, 24, 16)
GROWTH = 32
BN_SIZE = 4
INIT_FEATURES = 64


class _DenseLayer(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(cin)
        self.relu1 = nn.ReLU(inplace=True)
        self.conv1 = nn.Conv2d(cin, BN_SIZE * GROWTH, kernel_size=1, stride=1, bias=False)
        self.norm2 = nn.BatchNorm2d(BN_SIZE * GROWTH)
        self.relu2 = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(BN_SIZE * GROWTH, GROWTH, kernel_size=3, stride=1, padding=1, bias=False)

    def forward(self, x):
        y = self.conv1(self.relu1(self.norm1(x)))
        return self.conv2(self.relu2(self.norm2(y)))


class _DenseBlock(nn.ModuleDict):
    def __init__(self, nlayers, cin):
        super().__init__()
        self.cin = cin
        for i in range(nlayers):
            self.add_module(f"denselayer{i + 1}", _DenseLayer(cin + i * GROWTH))

    @property
    def cout(self):
        return self.cin + len(self) * GROWTH

    def forward(self, x):
        # one buffer for the whole block: layer i reads channels [0, cin + 32 i) and appends 32
        b, _, h, w = x.shape
        buf = x.new_empty((b, self.cout, h, w))
        buf[:, : self.cin] = x
        c = self.cin
        for layer in self.values():
            buf[:, c: c + GROWTH] = layer(buf[:, :c])
            c += GROWTH
        return buf


@dataclasses.dataclass(frozen=True)
class KernelConfig:
    """Which kernel family each piece of the inference path runs on.  FROZEN: a model holds one instance (`model.kernel_config`,
    every submodule carries a reference) and `model.configure(name=value, ..)` swaps in a modified copy -- no module-level
    switch, nothing another thread or another model instance can observe half-changed.  The defaults are the shipped path; the
    rest are measured alternatives kept for A/B runs and for inputs the default path does not cover."""
    densenet_two_fp16: bool = True          # DenseNet at 224 x 224: every conv on two fp16 terms, per-image value ranges
    plane_stride: tuple = ()                # ((side, floats between channel planes), ..): padded block buffers (measured: no gain)
    fused_small_maps: bool = False          # 14 x 14 / 7 x 7 dense layers in ONE launch (mirx_dense_layer_fused; slower so far)
    pooled_twin: bool = True                # DenseNet: the transition's norm + relu + avgpool of a layer's new channels written by its 3x3 launch
    hip_stem: bool = True                   # legacy (not 224 x 224) path: the stem kernel (False: torch ops)
    stem_three_bf16: bool = True            #   .. on three bf16 terms (False: fp32 MFMAs)
    hip_conv1x1: bool = True                #   fused 1x1 convs (False: rocBLAS via torch)
    conv1x1_three_bf16_min_cin: int = 0     #   1x1 convs with at least this many input channels on three bf16 terms
    hip_conv3x3: bool = True                #   own 3x3 convs on the 56 / 28 / 14 / 7 maps (False: MIOpen)
    conv3x3_legacy: tuple = ((56, "wino"), (28, "wino3"), (14, "direct3"), (7, "wino"))
    linear_three_bf16: bool = True          # token-major Linears on the MFMA kernels at all (False: rocBLAS fp32)
    linear_two_fp16: bool = True            #   .. on two fp16 terms where the input has a provable bound (LayerNorm outputs)
    cnx_grn_in_fc1: bool = True             #   .. and fc1's epilogue returns the GRN norm's partial sums (no norm pass over the hidden map)
    cnx_channels_last: bool = True          # ConvNeXtV2: the residual stream stays NHWC between blocks (no-LDS depthwise conv, row-major block tail)
    linear_terms_split_tail: bool = True    #   .. its last, partly filled round of tiles cut along K (mirx.h, mirx_linear_terms workspace)
    linear_terms_min_rows: int = 1024       #   .. ViT / SigLIP blocks with at least this many token rows: the DMA-fed Linear on pre-split
                                            #      "terms rows" (k_linear_t2: 256 x 256 tiles); 0 = never
    attention_three_bf16: bool = True       # flash attention on three bf16 terms (False: fp32 MFMAs)
    attention_two_fp16: bool = True         #   .. on two fp16 terms where q / k / v have provable bounds
    grn_scale_kernel: bool = True           # ConvNeXtV2: GRN scale vector + its maximum in one launch (False: five ATen launches)


DEFAULT_CONFIG = KernelConfig()


def _cfg(mod):
    """The kernel configuration a module runs under (its model's, or the defaults for a module used on its own)."""
    return getattr(mod, "_mirx_cfg", DEFAULT_CONFIG)


def set_kernel_config(module, cfg):
    """Put every submodule of `module` under `cfg` (what model.configure() does; also for a block used on its own)."""
    assert isinstance(cfg, KernelConfig)
    for m in module.modules():
        m.__dict__["_mirx_cfg"] = cfg
        # the duck-typed Linear views that are not nn.Modules (a patch-embedding / downsample conv seen as a Linear, SigLIP's
        # packed q / k / v rows): they run under their owner's configuration too
        for key in ("_mirx_as_linear", "_mirx_as_linear_cl", "_packed"):
            view = m.__dict__.get(key)
            if view is not None:
                view.__dict__["_mirx_cfg"] = cfg


class _Configurable:
    """Mixin of the top-level models: `kernel_config` and `configure(**changes)`."""

    def _init_config(self):
        set_kernel_config(self, DEFAULT_CONFIG)

    def _set_config(self, cfg):
        set_kernel_config(self, cfg)

    @property
    def kernel_config(self):
        return _cfg(self)

    def configure(self, **changes):
        """Swap in a copy of the configuration with `changes` applied; returns the previous configuration (to restore)."""
        old = _cfg(self)
        self._set_config(dataclasses.replace(old, **changes))
        return old


def _timer_start(timer):
    """Optional per-launch timing of the fused conv kernel (bench.py's calibration pass)."""
    if timer is None:
        return None
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    return ev


def _timer_stop(timer, ev, flops, nbytes=0.0, kind="conv1x1"):
    """(start event, stop event, FLOP, algorithmic bytes, kernel family) per launch."""
    if timer is not None:
        ev[1].record()
        timer.append((ev[0], ev[1], flops, nbytes, kind))


def _fused_bn_relu(lib, buf, c, scale, shift):
    """relu(bn(buf[:, :c])) -> packed [B, c, H, W] in one HIP pass over the channel-prefix view."""
    b, ctot, h, w = buf.shape
    out = torch.empty((b, c, h, w), dtype=torch.float32, device=buf.device)
    _lib.check(lib.mirx_bn_relu_nchw(_ptr(buf), ctot * h * w, _ptr(scale), _ptr(shift), b, c, h * w,
                                     _ptr(out), _stream(buf.device)), "mirx_bn_relu_nchw")
    return out


def _dense_block_fused(block, x, cache, cfg, timer=None):
    """Inference path of one dense block (CUDA, eval):
       per layer: [HIP] norm1+relu1 over the buffer prefix -> conv1 (1x1, norm2's scale folded into
       its weights) -> [HIP] norm2 shift + relu2 in place -> conv2 (3x3) -> 32 new channels copied
       into the block buffer."""
    lib = _lib.load()
    if isinstance(x, tuple):           # (block buffer, channels already in place): the transition wrote them there
        buf = x[0]
        x = buf
        b, _, h, w = buf.shape
    else:
        b, _, h, w = x.shape
        buf = torch.empty((b, block.cout, h, w), dtype=torch.float32, device=x.device)
        buf[:, : block.cin] = x
    c = block.cin
    for name, layer in block.items():
        sc1, sh1, w1, b1, ones, w1t, u3, w3 = cache[name]
        if cfg.hip_conv1x1:
            # norm1 + relu1 + conv1 + norm2 + relu2 in ONE fp32-MFMA pass over the buffer prefix
            y = torch.empty((b, w1t.shape[1], h, w), dtype=torch.float32, device=x.device)
            ev = _timer_start(timer)
            if c >= cfg.conv1x1_three_bf16_min_cin:
                # three-bf16-term MFMA formulation (fp32-grade, faster than the fp32-MFMA kernel on every layer)
                _lib.check(lib.mirx_conv1x1_bn_relu_split3(_ptr(buf), block.cout * h * w, c, _ptr(sc1), _ptr(sh1),
                                                           _ptr(w3), _ptr(b1), b, h * w, w1t.shape[1], 1, _ptr(y),
                                                           w1t.shape[1] * h * w, _stream(x.device)),
                           "mirx_conv1x1_bn_relu_split3")
            else:
                _lib.check(lib.mirx_conv1x1_bn_relu(_ptr(buf), block.cout * h * w, c, _ptr(sc1), _ptr(sh1), _ptr(w1t),
                                                    _ptr(b1), b, h * w, w1t.shape[1], 1, _ptr(y), _stream(x.device)),
                           "mirx_conv1x1_bn_relu")
            _timer_stop(timer, ev, 2.0 * b * h * w * c * w1t.shape[1])
            if cfg.hip_conv3x3 and h == w and h in (56, 28, 14, 7) and b <= 65535:
                # written straight into this layer's slice of the buffer.  Per map side (measured, 1024 images):
                # 56: Winograd F(2x2,3x3) on fp32 MFMAs (1.37 ms; the bf16 variants are operand-delivery bound there);
                # 28: Winograd on three-term bf16 MFMAs (0.32 vs 0.35 ms); 14: direct implicit GEMM on three-term
                # bf16 MFMAs (0.078 vs 0.090 / 0.097 ms); 7: Winograd fp32, two images per workgroup
                dst = ctypes.c_void_p(buf.data_ptr() + 4 * c * h * w)
                kind = dict(cfg.conv3x3_legacy).get(h, "wino")
                if kind == "direct3":
                    _lib.check(lib.mirx_conv3x3_direct_split3_nchw(_ptr(y), _ptr(u3[2]), b, h, dst, block.cout * h * w,
                                                                   _stream(x.device)), "mirx_conv3x3_direct_split3_nchw")
                elif kind == "wino3":
                    _lib.check(lib.mirx_conv3x3_winograd_split3_nchw(_ptr(y), _ptr(u3[1]), b, h, dst, block.cout * h * w,
                                                                     _stream(x.device)),
                               "mirx_conv3x3_winograd_split3_nchw")
                else:
                    _lib.check(lib.mirx_conv3x3_winograd_nchw(_ptr(y), _ptr(u3[0]), b, h, dst, block.cout * h * w,
                                                              _stream(x.device)), "mirx_conv3x3_winograd_nchw")
            else:
                buf[:, c: c + GROWTH] = F.conv2d(y, layer.conv2.weight, None, padding=1)
            c += GROWTH
            continue
        y = _fused_bn_relu(lib, buf, c, sc1, sh1)
        y = F.conv2d(y, w1)                       # norm2's scale is folded into w1 ...
        # ... and its shift + relu2 run as ONE in-place HIP pass (a conv bias would cost a separate
        # add kernel plus a clamp kernel under PyTorch-ROCm)
        _lib.check(lib.mirx_bn_relu_nchw(_ptr(y), y.shape[1] * h * w, _ptr(ones), _ptr(b1), b, y.shape[1], h * w,
                                         _ptr(y), _stream(y.device)), "mirx_bn_relu_nchw")
        y = F.conv2d(y, layer.conv2.weight, None, padding=1)
        buf[:, c: c + GROWTH] = y
        c += GROWTH
    return buf


def _transition_fused(tr, buf, cache, cfg, timer=None, next_channels=None):
    """[HIP] norm+relu+avgpool2x2 in one pass, then the 1x1 conv on the POOLED map (the conv and
    the average pool are both linear and commute; 4x fewer pixels go through the conv)."""
    lib = _lib.load()
    sc, sh, wt, w3 = cache
    b, c, h, w = buf.shape
    if h % 2 or w % 2:
        return tr.pool(tr.conv(F.relu(F.batch_norm(buf, tr.norm.running_mean, tr.norm.running_var,
                                                   tr.norm.weight, tr.norm.bias, False, 0.0, tr.norm.eps))))
    pooled = torch.empty((b, c, h // 2, w // 2), dtype=torch.float32, device=buf.device)
    _lib.check(lib.mirx_bn_relu_avgpool2(_ptr(buf), c * h * w, _ptr(sc), _ptr(sh), b, c, h, w, _ptr(pooled), 0,
                                         _stream(buf.device)), "mirx_bn_relu_avgpool2")
    if cfg.hip_conv1x1 and wt.shape[1] % 128 == 0 and c % 32 == 0:
        ev = _timer_start(timer)
        if c >= cfg.conv1x1_three_bf16_min_cin:
            # written straight into the channel prefix of the NEXT dense block's buffer when its width is known
            ctot = next_channels if next_channels else wt.shape[1]
            out = torch.empty((b, ctot, h // 2, w // 2), dtype=torch.float32, device=buf.device)
            _lib.check(lib.mirx_conv1x1_bn_relu_split3(_ptr(pooled), c * (h // 2) * (w // 2), c, None, None, _ptr(w3), None,
                                                       b, (h // 2) * (w // 2), wt.shape[1], 0, _ptr(out),
                                                       ctot * (h // 2) * (w // 2), _stream(buf.device)),
                       "mirx_conv1x1_bn_relu_split3")
            _timer_stop(timer, ev, 2.0 * b * (h // 2) * (w // 2) * c * wt.shape[1])
            return (out, wt.shape[1]) if next_channels else out
        else:
            out = torch.empty((b, wt.shape[1], h // 2, w // 2), dtype=torch.float32, device=buf.device)
            _lib.check(lib.mirx_conv1x1_bn_relu(_ptr(pooled), c * (h // 2) * (w // 2), c, None, None, _ptr(wt), None, b,
                                                (h // 2) * (w // 2), wt.shape[1], 0, _ptr(out), _stream(buf.device)),
                       "mirx_conv1x1_bn_relu")
        _timer_stop(timer, ev, 2.0 * b * (h // 2) * (w // 2) * c * wt.shape[1])
        return out
    return F.conv2d(pooled, tr.conv.weight)


def _plane_stride(side, cfg=DEFAULT_CONFIG):
    """Floats between consecutive channel planes of a dense block's buffer on the two-fp16-term path.
    784-byte (14 x 14) and 3136-byte (28 x 28) planes start at every 16-byte offset of a 128-byte line, so a wave's 256-byte
    load straddles three lines instead of two; in isolation the block-3 conv1x1 layers run at 4.1 instead of 3.5 TB/s on
    line-aligned planes (stride 224).  In the whole forward the padded layouts measured 1 % SLOWER (42.4 vs 42.8 k img/s,
    same box, B = 4096), so the default stays packed; the kernels and the ABI take the stride
    (KernelConfig.plane_stride, tools/bench_embed.py --plane-stride 14:224)."""
    hw = side * side
    ps = dict(cfg.plane_stride).get(side, hw)
    assert ps == hw or (ps > hw and ps % 4 == 0)
    return ps


def _dense_block_h2(block, buf, side, brange, cache, lranges, timer=None, fused_small=False, pool=None):
    """One dense block on the two-fp16-term kernels.  `buf` [B, block.cout, plane stride] (side x side pixels per plane, see
    _plane_stride) already holds the first block.cin channels and `brange` (range row [B]: one float per image) bounds them.
    56 / 28 maps, every layer: conv1x1 (norm1 + relu1 prologue, norm2 + relu2 epilogue) writes the bottleneck ALREADY SPLIT
    into fp16 terms, image b scaled by a bound derived from brange[b] before the kernel runs (2^-t goes to the layer's row of
    `lranges`); conv3x3 stages those terms by DMA, writes 32 channels into the buffer and folds their range into brange.
    14 / 7 maps with `fused_small`: ONE launch per layer, mirx_dense_layer_fused -- the bottleneck of a 196-pixel unit stays in
    the CU's LDS; bit-identical to the two launches and, so far, slower than them, hence opt-in.
    `pool` = (scale, shift, pooled) of the transition behind the block: every 3x3 launch then also writes norm + relu + avgpool2
    of its 32 new channels into `pooled` [B, block.cout, side/2, side/2] (mirx_conv3x3_direct_terms_nchw_pool; the caller has
    checked that the launches take the strip kernel)."""
    lib = _lib.load()
    b, _, ps = buf.shape
    h = w = side
    st = _stream(buf.device)
    c = block.cin
    fused = fused_small and side in (14, 7) and ps == h * w          # the fused kernel wants packed planes
    y = None if fused else torch.empty((b, BN_SIZE * GROWTH, h, w), dtype=torch.float32, device=buf.device)   # fp32 bytes, as terms
    for li, name in enumerate(block.keys()):
        e = cache[name]
        ev = _timer_start(timer)
        if fused:
            _lib.check(lib.mirx_dense_layer_fused(_ptr(buf), block.cout * ps, ps, c, _ptr(e["sc1"]), _ptr(e["sh1"]), _ptr(e["w2"]),
                                                  _ptr(e["osc"]), _ptr(e["b1"]), _ptr(e["c3w2p"]), _ptr(e["c3osc"]), b, side,
                                                  _ptr(brange), e["ks"], e["kb"], e["yks"], e["ykb"], st),
                       "mirx_dense_layer_fused")
            _timer_stop(timer, ev, 2.0 * b * h * w * (c * BN_SIZE * GROWTH + 9 * BN_SIZE * GROWTH * GROWTH),
                        4.0 * b * h * w * (c + GROWTH), "dense_fused")
            c += GROWTH
            continue
        dst = ctypes.c_void_p(buf.data_ptr() + 4 * c * ps)
        _lib.check(lib.mirx_conv1x1_bn_relu_split2h_terms(_ptr(buf), block.cout * ps, c, _ptr(e["sc1"]), _ptr(e["sh1"]),
                                                          _ptr(e["w2"]), _ptr(e["osc"]), _ptr(e["b1"]), b, h * w, _ptr(y),
                                                          _ptr(brange), e["ks"], e["kb"], e["yks"], e["ykb"],
                                                          _ptr(lranges[li]), ps, st), "mirx_conv1x1_bn_relu_split2h_terms")
        _timer_stop(timer, ev, 2.0 * b * h * w * c * y.shape[1], 4.0 * b * h * w * (c + y.shape[1]), "conv1x1")
        if pool is not None and not fused:
            psc, psh, pooled = pool
            hw2 = (h // 2) * (w // 2)
            _lib.check(lib.mirx_conv3x3_direct_terms_nchw_pool(_ptr(y), _ptr(e["c3w2p"]), _ptr(e["c3osc"]), b, h, dst,
                                                               block.cout * ps, _ptr(lranges[li]), _ptr(brange), ps,
                                                               ctypes.c_void_p(psc.data_ptr() + 4 * c),
                                                               ctypes.c_void_p(psh.data_ptr() + 4 * c),
                                                               ctypes.c_void_p(pooled.data_ptr() + 4 * c * hw2),
                                                               block.cout * hw2, st),
                       "mirx_conv3x3_direct_terms_nchw_pool")
        else:
            _lib.check(lib.mirx_conv3x3_direct_terms_nchw(_ptr(y), _ptr(e["c3w2p"]), _ptr(e["c3osc"]), b, h, dst,
                                                          block.cout * ps, _ptr(lranges[li]), _ptr(brange), ps, st),
                       "mirx_conv3x3_direct_terms_nchw")
        c += GROWTH
    return buf


def _transition_h2(buf, side, cache, brange, next_buf, next_range, timer=None, pooled=None, pooled_from=0):
    """norm -> relu -> avgpool2 -> conv 1x1 (the pool commutes with the linear conv; two fp16 terms; the pooled values are
    averages of relu(bn(x)), so max|scale| * range + max|shift| bounds them) written into the channel prefix of the next
    block's buffer [B, C', its plane stride], whose range row receives the output ranges: a bn + relu + avgpool pass feeds
    the plain 1x1 conv.  (A one-launch form with the pool inside the conv's staging measured equal in round 2 -- every
    128-channel output tile re-reads the un-pooled map -- and was dropped.)
    `pooled` given: the block's 3x3 launches have already written the channels from `pooled_from` on (their pooled twin);
    the pooling pass then covers only the block's first `pooled_from` channels."""
    lib = _lib.load()
    b, c, ps = buf.shape
    h = w = side
    st = _stream(buf.device)
    hw2 = (h // 2) * (w // 2)
    nps = next_buf.shape[2]
    if pooled is None:
        pooled = torch.empty((b, c, h // 2, w // 2), dtype=torch.float32, device=buf.device)
        _lib.check(lib.mirx_bn_relu_avgpool2(_ptr(buf), c * ps, _ptr(cache["sc"]), _ptr(cache["sh"]), b, c, h, w, _ptr(pooled), ps,
                                             st), "mirx_bn_relu_avgpool2")
    else:
        _lib.check(lib.mirx_bn_relu_avgpool2_into(_ptr(buf), c * ps, _ptr(cache["sc"]), _ptr(cache["sh"]), b, pooled_from, h, w,
                                                  _ptr(pooled), c * hw2, ps, st), "mirx_bn_relu_avgpool2_into")
    ev = _timer_start(timer)
    _lib.check(lib.mirx_conv1x1_bn_relu_split2h(_ptr(pooled), c * hw2, c, None, None, _ptr(cache["w2"]), _ptr(cache["osc"]),
                                                None, b, hw2, c // 2, 0, _ptr(next_buf), next_buf.shape[1] * nps,
                                                _ptr(brange), cache["ks"], cache["kb"], _ptr(next_range), 0, nps, st),
               "mirx_conv1x1_bn_relu_split2h")
    _timer_stop(timer, ev, 2.0 * b * hw2 * c * (c // 2), 4.0 * b * hw2 * (c + c // 2), "conv1x1")
    return next_buf


class _Transition(nn.Sequential):
    def __init__(self, cin, cout):
        super().__init__()
        self.norm = nn.BatchNorm2d(cin)
        self.relu = nn.ReLU(inplace=True)
        self.conv = nn.Conv2d(cin, cout, kernel_size=1, stride=1, bias=False)
        self.pool = nn.AvgPool2d(kernel_size=2, stride=2)


def _make_features():
    layers = OrderedDict()
    layers["conv0"] = nn.Conv2d(3, INIT_FEATURES, kernel_size=7, stride=2, padding=3, bias=False)
    layers["norm0"] = nn.BatchNorm2d(INIT_FEATURES)
    layers["relu0"] = nn.ReLU(inplace=True)
    layers["pool0"] = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
    c = INIT_FEATURES
    for i, n in enumerate(BLOCK_CONFIG):
        blk = _DenseBlock(n, c)
        layers[f"denseblock{i + 1}"] = blk
        c = blk.cout
        if i != len(BLOCK_CONFIG) - 1:
            layers[f"transition{i + 1}"] = _Transition(c, c // 2)
            c //= 2
    layers["norm5"] = nn.BatchNorm2d(c)
    feats = nn.Sequential(layers)
    for m in feats.modules():          # the published initialisation
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight)
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)
    return feats, c


def _winograd_weights(w):
    """conv2 weights [32, 128, 3, 3] -> U = G g G^T of Winograd F(2x2,3x3), laid out for
    mirx_conv3x3_winograd_nchw: [stage = c // 8][xi = 4 i + j][c % 8][oc], fp32."""
    g = w.detach().float()
    gm = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], device=g.device)
    u = torch.einsum("ik,ockl,jl->ocij", gm, g, gm)                       # [oc, c, 4, 4]
    oc, cin = u.shape[0], u.shape[1]
    u = u.reshape(oc, cin // 8, 8, 16).permute(1, 3, 2, 0)                # [stage, xi, c % 8, oc]
    return u.contiguous()


def _winograd_weights_split3(w):
    """conv2 weights [32, 128, 3, 3] -> the three bf16 terms of U = G g G^T, laid out for
    mirx_conv3x3_winograd_split3_nchw: [stage = c // 16][xi = 4 i + j][term][oc][c % 16] bf16."""
    g = w.detach().float()
    gm = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], device=g.device)
    u = torch.einsum("ik,ockl,jl->ocij", gm, g, gm)                       # [oc, c, 4, 4]
    h = u.to(torch.bfloat16)
    m = (u - h.float()).to(torch.bfloat16)
    lo = (u - h.float() - m.float()).to(torch.bfloat16)
    oc, cin = u.shape[0], u.shape[1]
    t = torch.stack([h, m, lo], 0).reshape(3, oc, cin // 16, 16, 16)      # [term, oc, stage, c % 16, xi]
    return t.permute(2, 4, 0, 1, 3).contiguous()


def _conv3x3_weights_split3(w):
    """conv2 weights [32, 128, 3, 3] -> the three bf16 terms laid out for mirx_conv3x3_direct_split3_nchw:
    [stage = c // 16][tap = 3 ky + kx][term][oc][c % 16] bf16."""
    w = w.detach().float()
    h = w.to(torch.bfloat16)
    m = (w - h.float()).to(torch.bfloat16)
    lo = (w - h.float() - m.float()).to(torch.bfloat16)
    oc, cin = w.shape[0], w.shape[1]
    t = torch.stack([h, m, lo], 0).reshape(3, oc, cin // 16, 16, 9)        # [term, oc, stage, c % 16, tap]
    return t.permute(2, 4, 0, 1, 3).contiguous()


# Channel order of the pre-split bottleneck (mirx_conv1x1_bn_relu_split2h_terms): slot j of group g holds channel
# 64 (g >> 2) + 32 ((g >> 1) & 1) + 4 (g & 1) + (j & 3) + 8 (j >> 2) -- the 16 channels one lane of the 1x1-conv kernel owns.
YTERMS_CHANNEL_ORDER = [64 * (g >> 2) + 32 * ((g >> 1) & 1) + 4 * (g & 1) + (j & 3) + 8 * (j >> 2)
                        for g in range(8) for j in range(16)]


def _conv3x3_weights_split2h(w, channel_order=None):
    """conv2 weights [32, 128, 3, 3] -> (w2, oscale): the two fp16 terms of W[oc] * ws[oc] (ws a power of two per output
    channel) laid out for mirx_conv3x3_direct_split2h_nchw: [stage = c // 16][tap = 3 ky + kx][term][oc][c % 16] fp16, and
    oscale = 1 / ws fp32 [32].  channel_order: input channels re-ordered first (YTERMS_CHANNEL_ORDER for the terms path)."""
    w = w.detach().float()
    if channel_order is not None:
        w = w[:, torch.as_tensor(channel_order, device=w.device)]
    oc, cin = w.shape[0], w.shape[1]
    ws = _pow2_row_scales(w.reshape(oc, -1))
    wf = w * ws.view(-1, 1, 1, 1)
    h = wf.to(torch.float16)
    lo = (wf - h.float()).to(torch.float16)
    t = torch.stack([h, lo], 0).reshape(2, oc, cin // 16, 16, 9)           # [term, oc, stage, c % 16, tap]
    return t.permute(2, 4, 0, 1, 3).contiguous(), (1.0 / ws).contiguous()


def _stem_weights_split3(w):
    """conv0 weights [64, 3, 7, 7] -> the three bf16 terms laid out for mirx_stem_conv7_bn_relu_pool_split3:
    [2 oc blocks][11 steps][term][32 oc][16 k]; k = 8 g + i of step s is row (c, ky) = divmod(2 s + g, 7) and
    kx = 0, 2, 4, 6, 1, 3, 5, (7 = zero) for i = 0..7; row 21 is zero."""
    w = w.detach().float()
    wk = torch.zeros((64, 22, 8), dtype=torch.float32, device=w.device)
    rows = w.reshape(64, 21, 7)                                            # [oc, (c, ky), kx]
    wk[:, :21, 0:4] = rows[:, :, 0::2]
    wk[:, :21, 4:7] = rows[:, :, 1::2]
    wk = wk.reshape(64, 11, 16)
    h = wk.to(torch.bfloat16)
    m = (wk - h.float()).to(torch.bfloat16)
    lo = (wk - h.float() - m.float()).to(torch.bfloat16)
    t = torch.stack([h, m, lo], 0).reshape(3, 2, 32, 11, 16)               # [term, block, oc, step, k]
    return t.permute(1, 3, 0, 2, 4).contiguous()


def _stem_weights_split2h(w):
    """conv0 weights [64, 3, 7, 7] -> (w2, oscale): the two fp16 terms of W[oc] * ws[oc] (a power of two per output channel)
    in the K order of mirx_stem_conv7_bn_relu_pool_split3 -- [2 oc blocks][11 steps][term][32 oc][16 k] -- and 1 / ws [64]."""
    w = w.detach().float()
    ws = _pow2_row_scales(w.reshape(64, -1))
    wk = torch.zeros((64, 22, 8), dtype=torch.float32, device=w.device)
    rows = (w * ws.view(-1, 1, 1, 1)).reshape(64, 21, 7)                   # [oc, (c, ky), kx]
    wk[:, :21, 0:4] = rows[:, :, 0::2]
    wk[:, :21, 4:7] = rows[:, :, 1::2]
    wk = wk.reshape(64, 11, 16)
    h = wk.to(torch.float16)
    lo = (wk - h.float()).to(torch.float16)
    t = torch.stack([h, lo], 0).reshape(2, 2, 32, 11, 16)                  # [term, block, oc, step, k]
    return t.permute(1, 3, 0, 2, 4).contiguous(), (1.0 / ws).contiguous()


def _split3_weights(w):
    """[cout, cin] fp32 -> the three bf16 terms of every weight (w = h + m + l exactly, 3 x 8 mantissa
    bits), laid out for mirx_conv1x1_bn_relu_split3: [cout // 128][cin // 16][3][128][16] bf16."""
    w = w.detach().float()
    if w.shape[0] % 128:                               # Linear layers: zero rows up to the next output tile
        w = F.pad(w, (0, 0, 0, 128 - w.shape[0] % 128))
    h = w.to(torch.bfloat16)
    m = (w - h.float()).to(torch.bfloat16)
    lo = (w - h.float() - m.float()).to(torch.bfloat16)
    cout, cin = w.shape
    t = torch.stack([h, m, lo], 0).reshape(3, cout // 128, 128, cin // 16, 16)
    return t.permute(1, 3, 0, 2, 4).contiguous()


def _pow2_row_scales(w):
    """Per output row of w [cout, k]: the power of two that puts the row's largest |w| in [2^13, 2^14) (so that the low
    fp16 term of all but vanishing weights stays a normal number); rows of zeros (or non-finite rows) get 1."""
    amax = w.abs().amax(dim=1)
    ok = torch.isfinite(amax) & (amax > 0)
    e = torch.floor(torch.log2(torch.where(ok, amax, torch.ones_like(amax))))
    # floor(log2) of an fp32 can be off by one at exact powers of two after rounding: fix up
    e = torch.where(torch.exp2(e) > amax, e - 1, e)
    e = torch.where(torch.exp2(e + 1) <= amax, e + 1, e)
    return torch.where(ok, torch.exp2(13 - e), torch.ones_like(amax))


def _split2h_weights(w):
    """[cout, cin] fp32 -> (w2, oscale): the two fp16 terms of W[o, :] * ws[o] (ws a power of two per output row),
    laid out for mirx_conv1x1_bn_relu_split2h: [cout // 128][cin // 16][2][128][16] fp16, and oscale = 1 / ws fp32."""
    w = w.detach().float()
    ws = _pow2_row_scales(w)
    wf = w * ws[:, None]
    h = wf.to(torch.float16)
    lo = (wf - h.float()).to(torch.float16)
    cout, cin = w.shape
    t = torch.stack([h, lo], 0).reshape(2, cout // 128, 128, cin // 16, 16)
    return t.permute(1, 3, 0, 2, 4).contiguous(), (1.0 / ws).contiguous()


def _bn_affine(bn):
    """Eval-mode BatchNorm as y = x*scale + shift (fp32)."""
    scale = bn.weight.detach().float() * torch.rsqrt(bn.running_var.detach().float() + bn.eps)
    shift = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
    return scale.contiguous(), shift.contiguous()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _linear_s3_ok(mod, x):
    return (_cfg(mod).linear_three_bf16 and x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled()
            and mod.in_features % 16 == 0)


def _tkey(t):
    """Cache key of a parameter: a replaced tensor object (load_state_dict(assign=True), `m.weight = nn.Parameter(..)`,
    `p.data = ..`) starts again at version 0, so the version alone would keep a stale entry alive."""
    return None if t is None else (id(t), t.data_ptr(), t._version)


def _cached_image(mod, slot, tensors, build):
    """build(): something derived from `tensors` (parameters, or None), kept in `mod.__dict__[slot]` and rebuilt when one
    of them changed (_tkey).  The entry holds the tensors it was built from: the id of a live object is not handed out again."""
    key = tuple(_tkey(t) for t in tensors)
    cached = mod.__dict__.get(slot)
    if cached is None or cached[0] != key:
        cached = (key, build(), tensors)
        mod.__dict__[slot] = cached
    return cached[1]


def _pow2_weight_scale(wf):
    """The power of two that puts the largest |w| in [2^13, 2^14) (so the low fp16 term stays a normal number)."""
    amax = float(wf.abs().max())
    return 2.0 ** math.floor(math.log2(16384.0 / amax)) if amax > 0 and math.isfinite(amax) else 1.0


def _linear_w3(mod):
    """The three-term bf16 image of a Linear's weight, rebuilt when the parameter changes."""
    return _cached_image(mod, "_mirx_w3", (mod.weight,), lambda: _split3_weights(mod.weight.detach()))


def _linear_h2_weights(mod):
    """(w2, w_scale): the two fp16 terms of W * w_scale (_pow2_weight_scale), laid out [ceil(n / 128)][k / 16][2][128][16]."""
    def build():
        wf = mod.weight.detach().float()
        ws = _pow2_weight_scale(wf)
        wf = wf * ws
        if wf.shape[0] % 128:
            wf = F.pad(wf, (0, 0, 0, 128 - wf.shape[0] % 128))
        wh = wf.to(torch.float16)
        wl = (wf - wh.float()).to(torch.float16)
        n, k = wf.shape
        t = torch.stack([wh, wl], 0).reshape(2, n // 128, 128, k // 16, 16)
        return t.permute(1, 3, 0, 2, 4).contiguous(), ws
    return _cached_image(mod, "_mirx_w2", (mod.weight,), build)


def _terms_of(a, scale):
    """Host-side "terms rows" of `a` [rows, k] * scale (include/mirx.h, mirx_linear_terms): fp16 [rows, ceil32(k) // 32, 2, 32]
    = per 32-feature group the high terms, then the low terms.  Used for weights (once per layer); activations are converted
    on the device (mirx_rows_to_terms, mirx_layernorm_terms, the terms output of mirx_linear_terms)."""
    a = a.float() * scale
    rows, k = a.shape
    if k % 32:
        a = F.pad(a, (0, 32 - k % 32))
    hi = a.to(torch.float16)
    lo = (a - hi.float()).to(torch.float16)
    return torch.stack([hi.view(rows, -1, 32), lo.view(rows, -1, 32)], 2).contiguous()


def _linear_terms_weights(mod):
    """(wt, w_scale): terms rows of W * w_scale (_pow2_weight_scale), rows padded to a multiple of 256 with zeros."""
    def build():
        wf = mod.weight.detach().float()
        ws = _pow2_weight_scale(wf)
        if wf.shape[0] % 256:
            wf = F.pad(wf, (0, 0, 0, 256 - wf.shape[0] % 256))
        return _terms_of(wf, ws), ws
    return _cached_image(mod, "_mirx_wt", (mod.weight,), build)


def _terms_scale(bound):
    """The power of two that brings |x| <= bound to at most 2^15 (fp16 terms overflow at 65504)."""
    return 2.0 ** math.floor(math.log2(32768.0 / bound))


def _rows_to_terms(x, bound):
    """[HIP] terms rows of x [..., k] (fp32, last axis contiguous) scaled for |x| <= bound -> (xt fp16 [m, ceil32(k) * 2], scale)."""
    k = x.shape[-1]
    x = x.reshape(-1, k)
    if x.stride(-1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16:
        x = x.contiguous()
    m = x.shape[0]
    xs = _terms_scale(bound)
    xt = torch.empty(m, (k + 31) // 32 * 64, dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mirx_rows_to_terms(_ptr(x), m, k, x.stride(0), xs, _ptr(xt), _stream(x.device)), "mirx_rows_to_terms")
    return xt, xs


def _layernorm_terms(ln, x, bound):
    """[HIP] LayerNorm over the last axis written as terms rows (the next Linear's input) -> (xt, scale)."""
    c = x.shape[-1]
    x = x.contiguous()
    m = x.numel() // c
    xs = _terms_scale(bound)
    xt = torch.empty(m, (c + 31) // 32 * 64, dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mirx_layernorm_terms(_ptr(x), m, c, _ptr(ln.weight.detach()) if ln.weight is not None else None,
                                                    _ptr(ln.bias.detach()) if ln.bias is not None else None, float(ln.eps), xs,
                                                    _ptr(xt), _stream(x.device)), "mirx_layernorm_terms")
    return xt, xs


def _linear_terms(mod, xt, xs, lead, act=0, res=None, gamma=None, out=None, terms_bound=None):
    """[HIP] y = epi(x W^T + b) through mirx_linear_terms; xt / xs = the input as terms rows and its scale, `lead` the
    leading shape of the result.  terms_bound: the result is returned as (terms rows, scale) for |y| <= terms_bound instead
    of fp32 (the fc1 -> fc2 hand-over)."""
    wt, ws = _linear_terms_weights(mod)
    m = xt.shape[0]
    n = mod.out_features
    dev = xt.device
    yt = ys = None
    if terms_bound is not None:
        ys = _terms_scale(terms_bound)
        yt = torch.empty(m, (n + 31) // 32 * 64, dtype=torch.float16, device=dev)
    elif out is None:
        out = torch.empty(tuple(lead) + (n,), dtype=torch.float32, device=dev)
    if res is not None:
        assert res.is_contiguous() and res.shape == out.shape
    lib = _lib.load()
    wsb = int(lib.mirx_linear_terms_workspace_bytes(m, mod.in_features, n)) if _cfg(mod).linear_terms_split_tail else 0
    wsp = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None         # stream-ordered: safe across streams
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mirx_linear_terms(_ptr(xt), m, mod.in_features, _ptr(wt),
                                                 _ptr(mod.bias.detach()) if mod.bias is not None else None, n, act,
                                                 _ptr(res) if res is not None else None,
                                                 _ptr(gamma.detach()) if gamma is not None else None, 1.0 / (xs * ws),
                                                 _ptr(out) if yt is None else None, _ptr(yt) if yt is not None else None,
                                                 ys if ys is not None else 1.0, _ptr(wsp) if wsp is not None else None, wsb,
                                                 _stream(dev)), "mirx_linear_terms")
    return (yt, ys) if yt is not None else out


def _linear_terms_ok(mod, rows, lins, bounds):
    """The DMA-fed Linear (mirx_linear_terms) serves a block when the batch fills its 256 x 256 tiles and every input has a
    provable bound (the same contract as _linear_h2_ok)."""
    cfg = _cfg(mod)
    return (cfg.linear_two_fp16 and cfg.linear_three_bf16 and cfg.linear_terms_min_rows > 0 and rows >= cfg.linear_terms_min_rows
            and all(l.out_features % 4 == 0 for l in lins) and all(math.isfinite(b) and 0.0 < b < 3.0e4 for b in bounds))


def _layernorm_bound(ln):
    """max |LayerNorm(x)_j| over all inputs: |x_j - mean| / std <= sqrt(C - 1), so sqrt(C - 1) max|gamma| + max|beta|."""
    g, b = ln.weight, ln.bias

    def build():
        c = ln.normalized_shape[-1]
        gm = 1.0 if g is None else float(g.detach().abs().max())
        bm = 0.0 if b is None else float(b.detach().abs().max())
        return math.sqrt(max(c - 1, 1)) * gm + bm
    return _cached_image(ln, "_mirx_bound", (g, b), build)


def _linear_out_bound(ln, lin, rows=None):
    """max |lin(LayerNorm(x))_j| over all inputs, for output rows `rows` (slice) of `lin`:
    ||LN(x)||_2 <= max|gamma| sqrt(C) + ||beta||_2 (the normalised vector has squared norm C), so
    |y_j| <= that * ||W_j||_2 + |b_j|.  GELU and softmax-weighted averages of such outputs obey the same bound."""
    g, b = ln.weight, ln.bias
    ver = (_tkey(g), _tkey(b), _tkey(lin.weight), _tkey(lin.bias))
    store = lin.__dict__.setdefault("_mirx_out_bound", {})
    if store.get("ver") != ver:                      # weights changed: every cached row range is stale
        store.clear()
        store["ver"] = ver
    key = None if rows is None else (rows.start, rows.stop)
    if key not in store:
        c = ln.normalized_shape[-1]
        gm = 1.0 if g is None else float(g.detach().abs().max())
        bn = 0.0 if b is None else float(torch.linalg.vector_norm(b.detach().double()))
        w = lin.weight.detach() if rows is None else lin.weight.detach()[rows]
        wn = float(torch.linalg.vector_norm(w.double(), dim=1).max())
        bb = 0.0 if lin.bias is None else float((lin.bias.detach() if rows is None else lin.bias.detach()[rows]).abs().max())
        store[key] = (gm * math.sqrt(c) + bn) * wn + bb
    return store[key]


def _linear_h2_ok(mod, x, bound):
    return (_cfg(mod).linear_two_fp16 and _linear_s3_ok(mod, x) and math.isfinite(bound) and 0.0 < bound < 3.0e4)


def _linear_h2(mod, x, bound, act=0, res=None, gamma=None, out=None):
    """[HIP] y = epi(x W^T + b) through mirx_linear_split2h; `bound` >= max |x| (the caller's proof obligation: fp16
    terms overflow at 65504) -- x is scaled by the power of two that brings `bound` to at most 2^15."""
    w2, ws = _linear_h2_weights(mod)
    xs = _terms_scale(bound)
    x = x.contiguous()
    m = x.numel() // mod.in_features
    if out is None:
        out = torch.empty(x.shape[:-1] + (mod.out_features,), dtype=torch.float32, device=x.device)
    if res is not None:
        assert res.is_contiguous() and res.shape == out.shape
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mirx_linear_split2h(_ptr(x), m, mod.in_features, _ptr(w2),
                                                   _ptr(mod.bias.detach()) if mod.bias is not None else None,
                                                   mod.out_features, act, _ptr(res) if res is not None else None,
                                                   _ptr(gamma.detach()) if gamma is not None else None,
                                                   xs, 1.0 / (xs * ws), _ptr(out), _stream(x.device)),
                   "mirx_linear_split2h")
    return out


def _linear_s3(mod, x, act=0, res=None, gamma=None, out=None):
    """[HIP] y = epi(x W^T + b) through mirx_linear_split3 (include/mirx.h); x: [..., k] fp32 CUDA.
    act=1: GELU; res/gamma: y = res + gamma * v (may be written in place with out=res)."""
    w3 = _linear_w3(mod)
    x = x.contiguous()
    m = x.numel() // mod.in_features
    if out is None:
        out = torch.empty(x.shape[:-1] + (mod.out_features,), dtype=torch.float32, device=x.device)
    if res is not None:
        assert res.is_contiguous() and res.shape == out.shape
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mirx_linear_split3(_ptr(x), m, mod.in_features, _ptr(w3),
                                                  _ptr(mod.bias.detach()) if mod.bias is not None else None,
                                                  mod.out_features, act, _ptr(res) if res is not None else None,
                                                  _ptr(gamma.detach()) if gamma is not None else None, _ptr(out),
                                                  _stream(x.device)), "mirx_linear_split3")
    return out


def _linear_bounded(mod, x, bound, act=0, res=None, gamma=None, out=None):
    """[HIP] y = epi(x W^T + b) for an input with max |x| <= bound: two fp16 terms where the bound is a proof they cannot
    overflow (_linear_h2_ok), three bf16 terms otherwise.  bound=None: nothing is known about x."""
    if bound is not None and _linear_h2_ok(mod, x, bound):
        return _linear_h2(mod, x, bound, act, res, gamma, out)
    return _linear_s3(mod, x, act, res, gamma, out)


def _linear_auto(mod, x, act=0):
    """nn.Linear forward that takes the MFMA kernel for CUDA fp32 inference (any [..., k] input, k % 16 == 0) and the
    module's own forward otherwise.  act: 0 none, 1 erf-GELU, 2 tanh-GELU (fused in the kernel's epilogue)."""
    if _linear_s3_ok(mod, x):
        return _linear_s3(mod, x, act=act)
    y = mod(x)
    return y if act == 0 else F.gelu(y, approximate="tanh" if act == 2 else "none")


def _layernorm(ln, x, tokens_per_image=0):
    """nn.LayerNorm over the last axis: [HIP] mirx_layernorm for CUDA fp32 inference, F.layer_norm otherwise.
    tokens_per_image > 0: x is [images * tpi, c] and the result comes back channels-first [images, c, tpi]."""
    c = ln.normalized_shape[-1]
    if (x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled() and c % 4 == 0 and c <= 8192
            and len(ln.normalized_shape) == 1 and x.shape[-1] == c):          # (the kernel keeps a row in registers: c <= 8192)
        x = x.contiguous()
        m = x.numel() // c
        if tokens_per_image:
            out = torch.empty((m // tokens_per_image, c, tokens_per_image), dtype=torch.float32, device=x.device)
        else:
            out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().mirx_layernorm(_ptr(x), m, c, _ptr(ln.weight.detach()) if ln.weight is not None else None,
                                                  _ptr(ln.bias.detach()) if ln.bias is not None else None, float(ln.eps),
                                                  _ptr(out), int(tokens_per_image), _stream(x.device)), "mirx_layernorm")
        return out
    y = F.layer_norm(x, ln.normalized_shape, ln.weight, ln.bias, ln.eps)
    if tokens_per_image:
        y = y.view(-1, tokens_per_image, c).transpose(1, 2).contiguous()
    return y


def _attention_packed(owner, qkv, heads, head_dim, scale, bqk, bv, terms_scale=None, key_mask=None, small_below=0,
                      fp32_fallback=False):
    """[HIP] softmax(q k^T * scale) v on a packed projection qkv [b, n, 3c] (fp32, contiguous; q | k | v, each heads x
    head_dim) under `owner`'s configuration.  bqk >= max |q|, |k| and bv >= max |v| (inf: no proof); key_mask [b, n]
    (1 = attend) or None.  -> (the context [b, n, c] fp32, False), or -- with terms_scale, where the two-fp16 flash kernel
    serves -- (the context * terms_scale as terms rows, fp16 [b * n, ceil32(c) * 2], True).
    Flash kernels (no mask, at least small_below tokens): two fp16 terms behind the bounds, else three bf16 terms -- or fp32
    MFMAs when fp32_fallback and the configuration turns attention_three_bf16 off.  Everything else: mirx_attention_small."""
    b, n, c = qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3
    cfg, dev, lib = _cfg(owner), qkv.device, _lib.load()
    flash = key_mask is None and n >= small_below and head_dim in (32, 64, 72, 96) and b <= 65535
    two_fp16 = flash and cfg.attention_two_fp16 and 0.0 < bqk < 3.0e4
    with torch.cuda.device(dev):
        st = _stream(dev)
        if two_fp16 and terms_scale is not None:
            # (a width that does not fill its last 32-feature group: the kernel leaves the padding to the allocation)
            ct = (torch.empty if c % 32 == 0 else torch.zeros)((b * n, (c + 31) // 32 * 64), dtype=torch.float16, device=dev)
            _lib.check(lib.mirx_attention_qkv_f32_split2h_terms(_ptr(qkv), b, n, heads, head_dim, scale, bqk, bv, terms_scale,
                                                                _ptr(ct), st), "mirx_attention_qkv_f32_split2h_terms")
            return ct, True
        ctx = torch.empty((b, n, c), dtype=torch.float32, device=dev)
        if two_fp16 and 0.0 < bv < 3.0e4:
            # q, k, v are outputs of a LayerNorm-fed Linear: provable bounds -> two fp16 terms per operand
            _lib.check(lib.mirx_attention_qkv_f32_split2h(_ptr(qkv), b, n, heads, head_dim, scale, bqk, bv, _ptr(ctx), st),
                       "mirx_attention_qkv_f32_split2h")
        elif flash and fp32_fallback and not cfg.attention_three_bf16:
            _lib.check(lib.mirx_attention_qkv_f32(_ptr(qkv), b, n, heads, head_dim, scale, _ptr(ctx), st), "mirx_attention_qkv_f32")
        elif flash:
            _lib.check(lib.mirx_attention_qkv_f32_split3(_ptr(qkv), b, n, heads, head_dim, scale, _ptr(ctx), st),
                       "mirx_attention_qkv_f32_split3")
        else:
            km = None if key_mask is None else key_mask.to(device=dev, dtype=torch.uint8).contiguous()
            base = qkv.data_ptr()
            _lib.check(lib.mirx_attention_small(ctypes.c_void_p(base), 3 * c, ctypes.c_void_p(base + 4 * c),
                                                ctypes.c_void_p(base + 8 * c), 3 * c, _ptr(km) if km is not None else None, b,
                                                heads, head_dim, n, n, scale, _ptr(ctx), st), "mirx_attention_small")
    return ctx, False


def _prenorm_block(owner, x, norm1, qkv, proj, norm2, fc1, fc2, heads, head_dim, scale, bqk, bv, bh, gelu, gamma1=None,
                   gamma2=None, key_mask=None, tap=None, small_below=0, fp32_fallback=False):
    """[HIP] The pre-norm transformer block of DINOv2 and the SigLIP towers, x [b, n, c] fp32:
        x = x + gamma1 * proj(attention(qkv(norm1(x))));  x = x + gamma2 * fc2(gelu(fc1(norm2(x))))
    in 4 MFMA Linear launches (bias / GELU / LayerScale + skip in their epilogues), one attention kernel and 2 LayerNorms.
    qkv: the packed projection (a Linear, or a view duck-typed as one); bqk, bv >= max |q|, |k| and max |v|, bh >= max |fc1(..)|
    over all inputs (the owner's proofs); gelu: 1 erf, 2 tanh; gamma1 / gamma2: LayerScale vectors or None; tap: None, or a
    callable handed the packed qkv [b, n, 3c] once it exists; small_below / fp32_fallback: as in _attention_packed."""
    b, n, c = x.shape
    x = x.contiguous()
    # the two Linears fed by a LayerNorm have a provable input bound; the context is a softmax-weighted average of V rows:
    # bounded like them (bv); |gelu(v)| <= |v| (bh)
    b1, b2 = _layernorm_bound(norm1), _layernorm_bound(norm2)
    # big batches: every Linear on the DMA-fed kernel, its input handed over as terms rows by the producer
    terms = _linear_terms_ok(owner, b * n, (qkv, proj, fc1, fc2), (b1, b2, bv, bh))
    if terms:
        h1t, s1 = _layernorm_terms(norm1, x, b1)
        qkv = _linear_terms(qkv, h1t, s1, (b, n))                                                     # [b, n, 3c]
    else:
        qkv = _linear_bounded(qkv, _layernorm(norm1, x), b1)
    if tap is not None:
        tap(qkv)
    sc = _terms_scale(bv) if terms else None
    ctx, is_terms = _attention_packed(owner, qkv, heads, head_dim, scale, bqk, bv, terms_scale=sc, key_mask=key_mask,
                                      small_below=small_below, fp32_fallback=fp32_fallback)
    if terms:
        ct = ctx if is_terms else _rows_to_terms(ctx, bv)[0]                       # (the same scale: _terms_scale(bv))
        x = _linear_terms(proj, ct, sc, (b, n), res=x, gamma=gamma1)
        h2t, s2 = _layernorm_terms(norm2, x, b2)
        hidt, sh = _linear_terms(fc1, h2t, s2, (b, n), act=gelu, terms_bound=bh)
        return _linear_terms(fc2, hidt, sh, (b, n), res=x, gamma=gamma2, out=x)
    x = _linear_bounded(proj, ctx, bv, res=x, gamma=gamma1)
    hid = _linear_bounded(fc1, _layernorm(norm2, x), b2, act=gelu)
    return _linear_bounded(fc2, hid, bh, res=x, gamma=gamma2, out=x)


class _ConvAsLinear:
    """A Conv2d whose kernel equals its stride (non-overlapping patches) seen as a Linear over patch rows: weight =
    conv.weight.flatten(1) zero-padded to a multiple of 16 input features (duck-typed for _linear_s3 / _linear_h2)."""

    def __init__(self, conv, channels_last=False):
        self.conv = conv
        self.channels_last = channels_last            # feature order (ky, kx, c): patch rows gathered from an NHWC map

    def refresh(self):
        w, b = self.conv.weight, self.conv.bias

        def build():
            flat = (w.detach().permute(0, 2, 3, 1) if self.channels_last else w.detach()).flatten(1)
            k = flat.shape[1]
            kp = (k + 15) // 16 * 16
            self.k, self.in_features, self.out_features = k, kp, flat.shape[0]
            self.weight = F.pad(flat, (0, kp - k)) if kp != k else flat.contiguous()
            self.bias = None if b is None else b.detach()
        _cached_image(self, "_mirx_view", (w, b), build)                 # (nothing to return: build() sets the view's attributes)
        return self


def _conv_patch_tokens(conv, x, ln2d=None, nchw_out=False):
    """[HIP] Conv2d(kernel = stride = p, no padding) on NCHW x as mirx_patchify_nchw + the MFMA Linear kernel.
    ln2d: an nn.LayerNorm applied over the channel axis of every pixel first (timm LayerNorm2d in front of the ConvNeXt
    downsample conv) -- its output is bounded, so the Linear runs on two fp16 terms.  -> [B * gh * gw, cout] rows, or the
    NCHW map [B, cout, gh, gw] when nchw_out."""
    pl = conv.__dict__.get("_mirx_as_linear")
    if pl is None:
        pl = _ConvAsLinear(conv)
        conv.__dict__["_mirx_as_linear"] = pl
    pl.__dict__["_mirx_cfg"] = _cfg(conv)          # the view runs under its conv's configuration
    pl.refresh()
    p = conv.kernel_size[0]
    b, c, h, w = x.shape
    gh, gw = h // p, w // p
    x = x.contiguous()
    rows = torch.empty((b * gh * gw, pl.in_features), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        st = _stream(x.device)
        _lib.check(lib.mirx_patchify_nchw(_ptr(x), b, c, h, w, p, _ptr(ln2d.weight.detach()) if ln2d is not None else None,
                                          _ptr(ln2d.bias.detach()) if ln2d is not None else None,
                                          float(ln2d.eps) if ln2d is not None else 0.0, _ptr(rows), pl.in_features, st),
                   "mirx_patchify_nchw")
        if nchw_out:
            out = torch.empty((b, pl.out_features, gh, gw), dtype=torch.float32, device=x.device)
            bound = _layernorm_bound(ln2d) if ln2d is not None else float("inf")
            if _linear_h2_ok(pl, rows, bound):                 # the rows are LayerNorm outputs: two fp16 terms
                w2, ws = _linear_h2_weights(pl)
                _lib.check(lib.mirx_linear_split2h_nchw(_ptr(rows), b, gh * gw, pl.in_features, _ptr(w2),
                                                        _ptr(pl.bias) if pl.bias is not None else None, pl.out_features, None,
                                                        None, float(bound), None, 1.0 / ws, _ptr(out), st),
                           "mirx_linear_split2h_nchw")
                return out
            _lib.check(lib.mirx_linear_split3_nchw(_ptr(rows), b, gh * gw, pl.in_features, _ptr(_linear_w3(pl)),
                                                   _ptr(pl.bias) if pl.bias is not None else None, pl.out_features, None, None,
                                                   _ptr(out), st), "mirx_linear_split3_nchw")
            return out
    return _linear_bounded(pl, rows, _layernorm_bound(ln2d) if ln2d is not None else None)


_TENSOR_VERSION = operator.attrgetter("_version")


class _InferenceCache:
    """Mixin of the models whose inference path runs on weights derived once from the parameters (folded BatchNorm, pre-split
    terms): `_cache()` returns the model's `_prepare_inference()` result and rebuilds it when any watched tensor changed.
    The model names the module whose parameters and buffers are watched (`_watch_root`)."""

    # The folded / pre-split weights are derived from the parameters and BatchNorm buffers; they are rebuilt whenever
    # any of those changed.  Routes that announce themselves drop the cache at once: load_state_dict (this module's own
    # and, through the pre-hook, a parent's), _apply (device moves, dtype casts), train().  What remains -- an in-place
    # edit of a parameter, a replaced tensor object -- is caught by ONE pass per forward over the watched tensors
    # (versions and identities: ~0.1 ms for DenseNet's 604 tensors; it was two passes of 0.22 ms, 18 % of a one-image forward).
    def _watch_lists(self):
        w = self.__dict__.get("_mirx_watch")
        if w is None:
            dicts, keys = [], []
            for m in self._watch_root().modules():
                for d in (m._parameters, m._buffers):
                    for k in d:
                        if d[k] is not None and k != "num_batches_tracked":       # not read by an eval-mode BatchNorm
                            dicts.append(d)
                            keys.append(k)
            w = (dicts, keys, [d[k] for d, k in zip(dicts, keys)])
            self.__dict__["_mirx_watch"] = w
        return w

    def _weights_version(self):
        """(sum of tensor versions, sum of tensor identities) over every parameter and BatchNorm buffer of the feature
        stack: in-place edits bump the first, a REPLACED tensor object (`conv.weight = nn.Parameter(..)`) changes the second."""
        dicts, keys, tens = self._watch_lists()
        ident = sum(map(id, map(dict.__getitem__, dicts, keys)))
        if ident != self.__dict__.get("_mirx_watch_ident"):
            self.__dict__.pop("_mirx_watch", None)                 # a tensor object was replaced: take the new objects
            dicts, keys, tens = self._watch_lists()
            self.__dict__["_mirx_watch_ident"] = ident = sum(map(id, tens))
        return sum(map(_TENSOR_VERSION, tens)), ident

    def _cache(self):
        ver = self._weights_version()
        cache = self._infer_cache
        if cache is None or cache.get("_version") != ver:
            cache = self._prepare_inference()
            cache["_version"] = ver
        if cache.get("_cuda"):
            # the folded / split weights are built by kernels on the stream that was current at the time; a stream that
            # has not seen them yet (bench.py's embed streams) waits for the newest build's event -- no device-wide sync
            sid = torch.cuda.current_stream().stream_id
            if sid not in cache["_seen"]:
                torch.cuda.current_stream().wait_event(cache["_built"])
                cache["_seen"].add(sid)
        return cache

    @staticmethod
    def _mark_built(cache):
        """Call after enqueueing work that fills `cache` on the current stream."""
        if cache.get("_cuda"):
            ev = torch.cuda.Event()
            ev.record()
            cache["_built"] = ev
            cache["_seen"] = {torch.cuda.current_stream().stream_id}

    def _drop_cache(self, *a, **k):
        self._infer_cache = None
        self.__dict__.pop("_mirx_watch", None)

    def train(self, mode=True):
        self._drop_cache()
        return super().train(mode)

    def load_state_dict(self, *a, **k):
        self._drop_cache()
        return super().load_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self._drop_cache()
        return super()._apply(fn, *a, **k)


class _OwnerRef:
    """A weak reference from a submodule to the model that owns it, kept in the submodule's __dict__ (outside the module tree
    and the state dict).  Pickling and deep copies drop it (a weakref can be neither pickled nor copied to the new model); the
    owner's __setstate__ puts one back that points at the new model."""
    __slots__ = ("_ref",)

    def __init__(self, owner=None):
        self._ref = weakref.ref(owner) if owner is not None else None

    def __call__(self):
        return self._ref() if self._ref is not None else None

    def __reduce__(self):
        return (_OwnerRef, ())

    def __deepcopy__(self, memo):
        return _OwnerRef()


class DenseNet121(_Configurable, _InferenceCache, nn.Module):
    """Reference model.py:42-84, MI355X-native inference path."""
    accepts_uint8 = True        # forward() takes raw 8-bit images and applies ToTensor + Normalize itself (input_mean / input_std)

    def __init__(self, pretrained=False, embedding_dim=None, num_labels=None, weights=None, _features=None):
        super().__init__()
        if pretrained and weights is None:
            raise RuntimeError("pretrained=True needs a download in the reference (model.py:53); "
                               "pass weights=<state dict or path> instead")
        feats, in_features = _make_features() if _features is None else (_features, _features.norm5.num_features)
        self.densenet121 = nn.Sequential(feats)
        # reference model.py:59-60: ReLU appended to the feature stack, avgpool to the wrapper
        if _features is None:
            self.densenet121[0].add_module("relu", nn.ReLU(inplace=True))
        self.densenet121.add_module("avgpool", nn.AdaptiveAvgPool2d((1, 1)))
        # SimCAM_Densenet121 is handed only the feature stack (or a Sequential of this model's children): it finds the model through
        # this weak reference, kept in __dict__ so it stays out of the module tree and the state dict
        self.densenet121[0].__dict__["_mirx_owner"] = _OwnerRef(self)
        self.fc = nn.Linear(in_features, embedding_dim) if embedding_dim else None
        out_features = embedding_dim if embedding_dim else in_features
        self.classification_head = nn.Linear(out_features, num_labels) if num_labels else None
        self.conv1x1_timer = None          # list -> (start event, stop event, FLOP) per fused conv launch
        # raw 8-bit input: forward() also takes uint8 [B, 3, H, W] and applies the reference's ToTensor + Normalize
        # (test.py:1309-1332) with these constants -- inside the stem kernel at 224 x 224, a quarter of the PCIe / HBM bytes
        self.register_buffer("input_mean", torch.tensor(IMAGENET_MEAN, dtype=torch.float32), persistent=False)
        self.register_buffer("input_std", torch.tensor(IMAGENET_STD, dtype=torch.float32), persistent=False)
        self._infer_cache = None           # folded BatchNorm parameters of the inference path
        self._init_config()
        if weights is not None:
            sd = torch.load(weights, map_location="cpu") if isinstance(weights, str) else weights
            for key in ("state-dict", "state_dict"):      # wrappers test.py:1273-1276 accepts
                if isinstance(sd, dict) and key in sd:
                    sd = sd[key]
            self.load_state_dict(sd, strict=False)

    @classmethod
    def _adopt(cls, features):
        """A headless DenseNet121 around an EXISTING feature stack (the same module objects: no parameter is copied) whose own
        model has been collected -- the reference's saliency drivers rebind `model` to a Sequential of its children, which drops
        the wrapper and keeps the stack.  The native feature path (_features_fused, _relu_rows) then runs on that stack again.
        The stack's owner reference points at the new model; the caller keeps the model alive."""
        owner = cls(_features=features)
        dev = features.conv0.weight.device
        owner.input_mean, owner.input_std = owner.input_mean.to(dev), owner.input_std.to(dev)
        owner.training = features.training           # the wrapper alone: the stack's own flags are not touched
        return owner

    def __setstate__(self, state):
        # unpickled or deep-copied: the feature stack's owner reference points at this model again
        super().__setstate__(state)
        feats = self.__dict__.get("_modules", {}).get("densenet121")
        if feats is not None and len(feats) > 0:
            feats[0].__dict__["_mirx_owner"] = _OwnerRef(self)

    # -- the plain module graph (training, CPU tensors): same ops as the reference -------------
    def forward_eager(self, x):
        x = self.densenet121(x)
        return torch.flatten(x, 1)

    # -- MI355X inference path -------------------------------------------------------------------
    def _watch_root(self):
        return self.densenet121[0]

    def _prepare_inference(self):
        """Fold every eval-mode BatchNorm once: norm1/transition norm -> (scale, shift) for the
        fused HIP passes; norm2 -> into conv1's weights and bias.  The operands of the legacy (three-bf16-term /
        Winograd) kernels are NOT built here: _ensure_legacy() does that when an input takes that path."""
        f = self.densenet121[0]
        cache = {}
        for name, m in f.named_children():
            if name.startswith("denseblock"):
                blk = {}
                for lname, layer in m.items():
                    sc1, sh1 = _bn_affine(layer.norm1)
                    sc2, sh2 = _bn_affine(layer.norm2)
                    w1 = (layer.conv1.weight.detach().float() * sc2.view(-1, 1, 1, 1)).contiguous()
                    w1t = w1.view(w1.shape[0], w1.shape[1]).t().contiguous()       # [cin, 128] for the HIP GEMM
                    blk[lname] = (sc1, sh1, w1, sh2, torch.ones_like(sh2), w1t, None, None)
                cache[name] = blk
            elif name.startswith("transition"):
                wt = m.conv.weight.detach().float()
                cache[name] = _bn_affine(m.norm) + (wt.view(wt.shape[0], wt.shape[1]).t().contiguous(), None)
        cache["norm0"] = _bn_affine(f.norm0)
        cache["norm5"] = _bn_affine(f.norm5)
        cache["_cuda"] = f.conv0.weight.is_cuda
        self._infer_cache = cache
        self._mark_built(cache)
        return cache

    def _ensure_legacy(self, cache):
        """Operands of the kernels that serve inputs other than 224 x 224 (three bf16 terms, Winograd): built on first use."""
        if cache.get("_legacy"):
            return
        f = self.densenet121[0]
        for name, m in f.named_children():
            if name.startswith("denseblock"):
                for lname, layer in m.items():
                    e = cache[name][lname]
                    w1 = e[2]
                    cache[name][lname] = e[:6] + ((_winograd_weights(layer.conv2.weight), _winograd_weights_split3(layer.conv2.weight),
                                                   _conv3x3_weights_split3(layer.conv2.weight)),
                                                  _split3_weights(w1.view(w1.shape[0], w1.shape[1])))
            elif name.startswith("transition"):
                wt = m.conv.weight.detach().float()
                cache[name] = cache[name][:3] + (_split3_weights(wt.view(wt.shape[0], wt.shape[1])),)
        cache["_legacy"] = True
        self._mark_built(cache)

    def _features_fused(self, x, cache):
        """-> (feature map before norm5 [B,1024,h,w])"""
        f = self.densenet121[0]
        lib = _lib.load()
        if x.dtype == torch.uint8:
            if self._h2_ok(x):
                return self._features_h2(x.contiguous(), cache)          # normalised inside the stem kernel
            x = self.normalize_uint8(x)
        x = x.contiguous().float()
        b, _, h, w = x.shape
        if self._h2_ok(x):
            return self._features_h2(x, cache)
        self._ensure_legacy(cache)
        cfg = _cfg(self)
        if cfg.hip_stem and h % 4 == 0 and w % 4 == 0 and h >= 8 and w >= 8:
            sc, sh = cache["norm0"]
            y = torch.empty((b, INIT_FEATURES, h // 4, w // 4), dtype=torch.float32, device=x.device)
            if cfg.stem_three_bf16 and b <= 65535:
                if "conv0_w3" not in cache:
                    cache["conv0_w3"] = _stem_weights_split3(f.conv0.weight)
                    self._mark_built(cache)
                _lib.check(lib.mirx_stem_conv7_bn_relu_pool_split3(_ptr(x), _ptr(cache["conv0_w3"]), _ptr(sc), _ptr(sh),
                                                                   b, h, w, _ptr(y), _stream(x.device)), "mirx_stem_split3")
            else:
                wt = f.conv0.weight.detach().float().contiguous()
                _lib.check(lib.mirx_stem_conv7_bn_relu_pool(_ptr(x), _ptr(wt), _ptr(sc), _ptr(sh), b, h, w,
                                                            _ptr(y), _stream(x.device)), "mirx_stem")
            x = y
        else:
            x = f.pool0(f.relu0(f.norm0(f.conv0(x))))
        children = list(f.named_children())
        for i, (name, m) in enumerate(children):
            if name.startswith("denseblock"):
                x = _dense_block_fused(m, x, cache[name], cfg, self.conv1x1_timer)
            elif name.startswith("transition"):
                nxt = children[i + 1][1] if i + 1 < len(children) and children[i + 1][0].startswith("denseblock") else None
                x = _transition_fused(m, x, cache[name], cfg, self.conv1x1_timer, nxt.cout if nxt is not None else None)
        return x

    def normalize_uint8(self, x):
        """ToTensor + Normalize of the reference (test.py:1309-1332) on a uint8 [B, 3, H, W] batch, the same fp32 operations in
        the same order (u / 255, - mean, / std): what the stem kernel's table holds."""
        m = self.input_mean.to(x.device).view(1, 3, 1, 1)
        s_ = self.input_std.to(x.device).view(1, 3, 1, 1)
        return (x.float() / 255.0 - m) / s_

    def _h2_ok(self, x):
        """The two-fp16-term path covers the geometry of the reference's 224 x 224 evaluation (maps 56 / 28 / 14 / 7)."""
        cfg = _cfg(self)
        return (cfg.densenet_two_fp16 and cfg.hip_stem and cfg.hip_conv1x1 and cfg.hip_conv3x3 and cfg.stem_three_bf16
                and x.shape[-1] == 224 and x.shape[-2] == 224 and 0 < x.shape[0] <= 65535)

    def _prepare_h2(self, cache):
        """Per layer: conv1 (norm2 folded) and conv2 as two fp16 terms with per-output-channel scales, and the host
        constants max |norm1 scale| / max |norm1 shift| that turn the buffer's published range into a bound."""
        f = self.densenet121[0]
        h2 = {}
        for name, m in f.named_children():
            if name.startswith("denseblock"):
                blk = {}
                for lname, layer in m.items():
                    sc1, sh1, w1, b1 = cache[name][lname][0], cache[name][lname][1], cache[name][lname][2], cache[name][lname][3]
                    w2, osc = _split2h_weights(w1.view(w1.shape[0], w1.shape[1]))
                    c3w2p, c3osc = _conv3x3_weights_split2h(layer.conv2.weight, YTERMS_CHANNEL_ORDER)
                    blk[lname] = {"sc1": sc1, "sh1": sh1, "b1": b1, "w2": w2, "osc": osc, "c3osc": c3osc,
                                  "c3w2p": c3w2p, "ks": float(sc1.abs().max()),
                                  "kb": float(sh1.abs().max()),
                                  # |relu(W x + b)| <= max_o sum_c |W[o, c]| * max|x| + max|b|: the bottleneck's bound
                                  "yks": float(w1.view(w1.shape[0], -1).abs().sum(dim=1).max()), "ykb": float(b1.abs().max())}
                h2[name] = blk
            elif name.startswith("transition"):
                sc, sh = cache[name][0], cache[name][1]
                wt = m.conv.weight.detach().float()
                w2, osc = _split2h_weights(wt.view(wt.shape[0], wt.shape[1]))
                h2[name] = {"sc": sc, "sh": sh, "w2": w2, "osc": osc, "ks": float(sc.abs().max()), "kb": float(sh.abs().max())}
        cache["conv0_w2"] = _stem_weights_split2h(f.conv0.weight)
        cache["h2"] = h2
        self._mark_built(cache)
        return h2

    def _features_h2(self, x, cache):
        """-> feature map before norm5 [B, 1024, 7, 7]; every convolution on the matrix pipe with two fp16 terms per
        operand, ranges carried in range slots."""
        f = self.densenet121[0]
        lib = _lib.load()
        h2 = cache.get("h2") or self._prepare_h2(cache)
        cfg = _cfg(self)
        u8 = x.dtype == torch.uint8
        x = x.contiguous() if u8 else x.contiguous().float()
        b = x.shape[0]
        dev = x.device
        st = _stream(dev)
        blocks = [(n, m) for n, m in f.named_children() if n.startswith("denseblock")]
        trans = [n for n, _ in f.named_children() if n.startswith("transition")]
        nlayers = sum(len(m) for _, m in blocks)
        # range rows: one float per (buffer, image) -- the blocks' buffers, every layer's bottleneck scale, the input images
        ranges = torch.zeros((len(blocks) + nlayers + 1, b), dtype=torch.float32, device=dev)   # one fill per forward
        sc, sh = cache["norm0"]
        xr = ranges[len(blocks) + nlayers]                           # the range of every input image: one pass over them
        if u8:
            _lib.check(lib.mirx_range_absmax_u8(_ptr(x), 224 * 224, b, _ptr(self.input_mean), _ptr(self.input_std), _ptr(xr), st),
                       "mirx_range_absmax_u8")
        else:
            _lib.check(lib.mirx_range_absmax(_ptr(x), x[0].numel(), b, _ptr(xr), st), "mirx_range_absmax")
        w2, osc = cache["conv0_w2"]
        sides = [56 >> k for k in range(len(blocks))]
        rows = [len(blocks) + sum(len(m) for _, m in blocks[:k]) for k in range(len(blocks))]

        def stem(xs, dst):
            if u8:
                _lib.check(lib.mirx_stem_conv7_bn_relu_pool_split2h_u8_into(_ptr(xs), _ptr(self.input_mean), _ptr(self.input_std),
                                                                            _ptr(w2), _ptr(osc), _ptr(sc), _ptr(sh), xs.shape[0],
                                                                            224, 224, _ptr(dst), dst.shape[1] * dst.shape[2],
                                                                            _ptr(xr), _ptr(ranges[0]), st),
                           "mirx_stem_split2h_u8_into")
                return
            _lib.check(lib.mirx_stem_conv7_bn_relu_pool_split2h_into(_ptr(xs), _ptr(w2), _ptr(osc), _ptr(sc), _ptr(sh),
                                                                     xs.shape[0], 224, 224, _ptr(dst),
                                                                     dst.shape[1] * dst.shape[2], _ptr(xr), _ptr(ranges[0]), st),
                       "mirx_stem_split2h_into")

        def block_and_transition(k, bk, nxt):
            name, blk = blocks[k]
            # the transition's norm + relu + avgpool of every NEW channel comes out of the 3x3 launch that writes it (its pooled
            # twin: the strip kernel only, so not for launches small enough for the one-wave-per-block kernel)
            pool = None
            if (nxt is not None and cfg.pooled_twin and not (cfg.fused_small_maps and sides[k] in (14, 7))
                    and not lib.mirx_conv3x3_small_launch(bk.shape[0], sides[k])):
                t = h2[trans[k]]
                pool = (t["sc"], t["sh"], torch.empty((bk.shape[0], blk.cout, sides[k] // 2, sides[k] // 2),
                                                      dtype=torch.float32, device=dev))
            _dense_block_h2(blk, bk, sides[k], ranges[k], h2[name], ranges[rows[k]:rows[k] + len(blk)], self.conv1x1_timer,
                            cfg.fused_small_maps, pool)
            if nxt is not None:
                _transition_h2(bk, sides[k], h2[trans[k]], ranges[k], nxt, ranges[k + 1], self.conv1x1_timer,
                               pool[2] if pool else None, blk.cin)

        def new_buf(k, n):
            return torch.empty((n, blocks[k][1].cout, _plane_stride(sides[k], cfg)), dtype=torch.float32, device=dev)

        buf = new_buf(0, b)
        stem(x, buf)
        for k in range(len(blocks)):
            nxt = new_buf(k + 1, b) if k + 1 < len(blocks) else None
            block_and_transition(k, buf, nxt)
            if nxt is not None:
                buf = nxt
        side = sides[-1]
        buf = buf.view(b, buf.shape[1], side, side)                 # the 7 x 7 planes are packed
        self.__dict__["_mirx_last_ranges"] = ranges            # kept for diagnostics (tools/h2_state_probe.py)
        return buf

    def _relu_rows(self, x, cache):
        """[HIP] the map of densenet121[0].relu (norm5 + ReLU) as channels-last rows [B, h * w, 1024] -> (rows, h, w): the
        feature map SimCAM_Densenet121 decomposes.  _features_fused, then norm5 + ReLU + NCHW -> rows in one pass."""
        fmap = self._features_fused(x, cache).contiguous()
        b, c, h, w = fmap.shape
        sc, sh = cache["norm5"]
        rows = torch.empty((b, h * w, c), dtype=torch.float32, device=fmap.device)
        _lib.check(_lib.load().mirx_bn_relu_rows(_ptr(fmap), b, c, h * w, _ptr(sc), _ptr(sh), _ptr(rows), _stream(fmap.device)),
                   "mirx_bn_relu_rows")
        return rows, h, w

    def _head_fused(self, fmap, normalize, cache=None):
        lib = _lib.load()
        sc, sh = (cache or self._cache())["norm5"]
        fmap = fmap.contiguous()
        b, c, h, w = fmap.shape
        out = torch.empty((b, c), dtype=torch.float32, device=fmap.device)
        _lib.check(lib.mirx_bn_relu_gap_l2norm(_ptr(fmap), _ptr(sc), _ptr(sh), b, c, h * w,
                                               1 if normalize else 0, _ptr(out), _stream(fmap.device)),
                   "mirx_bn_relu_gap_l2norm")
        return out

    def forward(self, x):
        fused = x.is_cuda and not self.training and not torch.is_grad_enabled()
        if fused:
            with torch.cuda.device(x.device):
                cache = self._cache()                  # ONE validity check of the folded weights per forward
                fmap = self._features_fused(x, cache)
                plain_head = self.fc is None and self.classification_head is None
                x = self._head_fused(fmap, normalize=plain_head, cache=cache)
                if plain_head:
                    return x                       # already unit-norm (model.py:83)
        else:
            x = self.forward_eager(self.normalize_uint8(x) if x.dtype == torch.uint8 else x)
        if self.fc:
            x = _linear_auto(self.fc, x)         # [HIP] three-bf16-term Linear on the inference path: no library GEMM in a forward
        if self.classification_head is not None:
            return {"embedding": F.normalize(x, dim=1), "logits": self.classification_head(x)}
        return F.normalize(x, dim=1)


# =================================================================================================
# ConvNeXtV2-base (reference model.py:87-117 around timm 'convnextv2_base.fcmae_ft_in22k_in1k_384',
# num_classes=0).  timm is not a dependency: the module tree below reproduces its parameter names
# (stem.0/1, stages.N.downsample.0/1, stages.N.blocks.M.{conv_dw,norm,mlp.fc1,mlp.grn,mlp.fc2},
# head.norm) so reference checkpoints (`convnext.*`, `fc.*`) load unchanged.
# =================================================================================================
CNX_DEPTHS = (3, 3, 27, 3)
CNX_DIMS = (128, 256, 512, 1024)
CNX_EPS = 1e-6


class _LayerNorm2d(nn.LayerNorm):
    """LayerNorm over the channel axis of an NCHW tensor (timm LayerNorm2d)."""

    def forward(self, x):
        return F.layer_norm(x.permute(0, 2, 3, 1), self.normalized_shape, self.weight, self.bias,
                            self.eps).permute(0, 3, 1, 2)


class _GRN(nn.Module):
    """Global response normalisation on NHWC (timm GlobalResponseNorm, channels_last)."""

    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(dim))
        self.bias = nn.Parameter(torch.zeros(dim))

    def forward(self, x):
        g = torch.linalg.vector_norm(x, ord=2, dim=(1, 2), keepdim=True)
        n = g / (g.mean(dim=-1, keepdim=True) + 1e-6)
        return x + torch.addcmul(self.bias, self.weight, x * n)


class _CnxMlp(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.grn = _GRN(4 * dim)
        self.fc2 = nn.Linear(4 * dim, dim)

    def forward(self, x):
        if _linear_s3_ok(self.fc1, x) and _linear_s3_ok(self.fc2, x):
            return _linear_s3(self.fc2, self.grn(_linear_s3(self.fc1, x, act=1)))      # bias + GELU in the epilogue
        return self.fc2(self.grn(self.act(self.fc1(x))))


class _CnxBlock(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.conv_dw = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=CNX_EPS)
        self.mlp = _CnxMlp(dim)

    def _fc2_bias_with_grn_shift(self):
        fc2, grn = self.mlp.fc2, self.mlp.grn
        key = (fc2.weight.data_ptr(), fc2.weight._version, grn.bias._version,
               None if fc2.bias is None else fc2.bias._version, fc2.weight.device)
        cached = getattr(self, "_mirx_bias2", None)
        if cached is None or cached[0] != key:
            bias = (fc2.weight.detach().double() @ grn.bias.detach().double()).float()
            if fc2.bias is not None:
                bias = bias + fc2.bias.detach()
            cached = (key, bias.contiguous())
            self._mirx_bias2 = cached
        return cached[1]

    def _forward_nhwc(self, t, b, h, w):
        """[HIP] The block on a channels-last residual stream t [b * h * w, c] (ConvNeXtV2 fast path): depthwise 7x7 without
        LDS (a lane = a channel), LayerNorm, fc1 + GELU, GRN as a norm pass + a scale folded into fc2's staging, fc2 with the
        skip added in its row-major epilogue.  -> the new stream (a fresh tensor)."""
        lib = _lib.load()
        mlp, c, dev = self.mlp, t.shape[-1], t.device
        wk = self.conv_dw.weight
        key = _tkey(wk)
        cached = getattr(self, "_mirx_dw_t", None)
        if cached is None or cached[0] != key:
            cached = (key, wk.detach().reshape(c, 49).t().contiguous())          # [49][c]: a lane reads its channel's taps coalesced
            self._mirx_dw_t = cached
        y = torch.empty_like(t)
        with torch.cuda.device(dev):
            _lib.check(lib.mirx_dwconv7x7_nhwc(_ptr(t), _ptr(cached[1]), _ptr(self.conv_dw.bias.detach()), b, c, h, w, _ptr(y),
                                               _stream(dev)), "mirx_dwconv7x7_nhwc")
        yn = _layernorm(self.norm, y)
        bn = _layernorm_bound(self.norm)
        c4 = mlp.fc1.out_features
        gx = torch.empty((b, c4), dtype=torch.float32, device=dev)
        fused_norm = h * w >= 128 and _cfg(self).cnx_grn_in_fc1
        if fused_norm:
            # fc1 + GELU returns the GRN partial sums of its own output tiles: the norm pass over the 4C-wide map disappears
            w2f, wsf = _linear_h2_weights(mlp.fc1)
            xs = _terms_scale(bn)
            hid = torch.empty((b * h * w, c4), dtype=torch.float32, device=dev)   # [b * h * w, 4c]
            parts = torch.empty(((b * h * w + 127) // 128) * 2 * c4, dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                _lib.check(lib.mirx_linear_split2h_gelu_grn(_ptr(yn), b, h * w, c, _ptr(w2f), _ptr(mlp.fc1.bias.detach()), c4, xs,
                                                            1.0 / (xs * wsf), _ptr(hid), _ptr(parts), _ptr(gx), _stream(dev)),
                           "mirx_linear_split2h_gelu_grn")
        else:
            hid = _linear_h2(mlp.fc1, yn, bn, act=1)                              # [b * h * w, 4c]
        scale = torch.empty_like(gx)
        smax = torch.zeros(1, dtype=torch.float32, device=dev)
        out = torch.empty_like(t)
        w2, ws = _linear_h2_weights(mlp.fc2)
        hb = _linear_out_bound(self.norm, mlp.fc1)                                # |gelu(fc1(LN(.)))| <= hb
        with torch.cuda.device(dev):
            st = _stream(dev)
            if not fused_norm:
                _lib.check(lib.mirx_grn_norm_nhwc(_ptr(hid), b, h * w, c4, _ptr(gx), st), "mirx_grn_norm_nhwc")
            _lib.check(lib.mirx_grn_scale(_ptr(gx), _ptr(mlp.grn.weight.detach().reshape(-1).contiguous()), b, c4, 1e-6,
                                          _ptr(scale), _ptr(smax), st), "mirx_grn_scale")
            _lib.check(lib.mirx_linear_split2h_grn_rows(_ptr(hid), b, h * w, c4, _ptr(w2), _ptr(self._fc2_bias_with_grn_shift()), c,
                                                        _ptr(t), _ptr(scale), float(hb), _ptr(smax), 1.0 / ws, _ptr(out), st),
                       "mirx_linear_split2h_grn_rows")
        return out

    def _nhwc_ok(self):
        mlp = self.mlp
        bn = _layernorm_bound(self.norm)
        hb = _linear_out_bound(self.norm, mlp.fc1)
        probe = self.conv_dw.weight
        return (_cfg(self).grn_scale_kernel and probe.is_cuda and self.conv_dw.bias is not None and mlp.fc1.bias is not None
                and _linear_h2_ok(mlp.fc1, probe, bn) and _linear_h2_ok(mlp.fc2, probe, hb))

    def forward(self, x):
        if x.is_cuda and not torch.is_grad_enabled() and x.dtype == torch.float32:
            # MI355X path: depthwise 7x7 + the NCHW->NHWC permute in one HIP pass
            lib = _lib.load()
            xc = x.contiguous()
            b, c, h, w = xc.shape
            y = torch.empty((b, h, w, c), dtype=torch.float32, device=x.device)
            with torch.cuda.device(x.device):
                _lib.check(lib.mirx_dwconv7x7_nchw_to_nhwc(_ptr(xc), _ptr(self.conv_dw.weight.detach().contiguous()),
                                                           _ptr(self.conv_dw.bias.detach().contiguous()), b, c, h, w,
                                                           _ptr(y), _stream(x.device)), "mirx_dwconv7x7")
        else:
            y = self.conv_dw(x).permute(0, 2, 3, 1)
        mlp = self.mlp
        if (x.is_cuda and y.is_contiguous() and x.shape[0] <= 65535 and _linear_s3_ok(mlp.fc1, y)
                and _linear_s3_ok(mlp.fc2, y)):
            # MI355X path: fc1 + GELU in one MFMA launch, GRN = one norm pass + a scale folded into fc2's staging,
            # fc2 written back NCHW with the skip added in its epilogue
            lib = _lib.load()
            b, c, h, w = x.shape
            yn = _layernorm(self.norm, y)
            bn = _layernorm_bound(self.norm)                               # fc1 reads a LayerNorm output
            hid = _linear_bounded(mlp.fc1, yn, bn, act=1)                  # [b, h, w, 4c]
            c4 = hid.shape[-1]
            gx = torch.empty((b, c4), dtype=torch.float32, device=x.device)
            out = torch.empty_like(xc)
            with torch.cuda.device(x.device):
                st = _stream(x.device)
                _lib.check(lib.mirx_grn_norm_nhwc(_ptr(hid), b, h * w, c4, _ptr(gx), st), "mirx_grn_norm_nhwc")
                if _cfg(self).grn_scale_kernel:
                    scale = torch.empty_like(gx)
                    smax = torch.zeros(1, dtype=torch.float32, device=x.device)
                    _lib.check(lib.mirx_grn_scale(_ptr(gx), _ptr(mlp.grn.weight.detach().reshape(-1).contiguous()), b, c4, 1e-6,
                                                  _ptr(scale), _ptr(smax), st), "mirx_grn_scale")
                else:                                                      # the ATen expression of the same vector (A/B)
                    scale = torch.addcmul(torch.ones_like(gx), mlp.grn.weight.detach(),
                                          gx / (gx.mean(dim=-1, keepdim=True) + 1e-6))
                    smax = scale.abs().amax().reshape(1)
                # GRN apply folded into the second Linear: the scale multiplies x while it is staged, the shift
                # is constant per feature, so W (x s + b) + bias = W (x s) + (bias + W b)
                hb = _linear_out_bound(self.norm, mlp.fc1)                 # |gelu(fc1(LN(.)))| <= |fc1(LN(.))| <= hb
                if _linear_h2_ok(mlp.fc2, hid, hb):
                    # two fp16 terms: |hid * scale| <= hb * max |scale|; the second factor is data, so it stays on the
                    # device (one scalar) and the kernel derives its staging scale from it
                    w2, ws = _linear_h2_weights(mlp.fc2)
                    _lib.check(lib.mirx_linear_split2h_nchw(_ptr(hid), b, h * w, c4, _ptr(w2),
                                                            _ptr(self._fc2_bias_with_grn_shift()), c, _ptr(xc), _ptr(scale),
                                                            float(hb), _ptr(smax), 1.0 / ws, _ptr(out), st),
                               "mirx_linear_split2h_nchw")
                else:
                    _lib.check(lib.mirx_linear_split3_nchw(_ptr(hid), b, h * w, c4, _ptr(_linear_w3(mlp.fc2)),
                                                           _ptr(self._fc2_bias_with_grn_shift()), c, _ptr(xc), _ptr(scale),
                                                           _ptr(out), st), "mirx_linear_split3_nchw")
            return out
        y = self.mlp(self.norm(y))
        return y.permute(0, 3, 1, 2) + x


class _CnxStage(nn.Module):
    def __init__(self, cin, cout, depth, downsample):
        super().__init__()
        if downsample:
            self.downsample = nn.Sequential(_LayerNorm2d(cin, eps=CNX_EPS), nn.Conv2d(cin, cout, kernel_size=2, stride=2))
        else:
            self.downsample = nn.Identity()
        self.blocks = nn.Sequential(*[_CnxBlock(cout) for _ in range(depth)])

    def forward(self, x):
        ds = self.downsample
        if (isinstance(ds, nn.Sequential) and x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled()
                and x.shape[0] <= 65535 and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0 and _cfg(self).linear_three_bf16):
            # MI355X path: LayerNorm2d + the NCHW -> patch-row gather in one HIP pass, the 2x2/2 conv as an MFMA Linear
            # that writes the next stage's NCHW map
            x = _conv_patch_tokens(ds[1], x, ln2d=ds[0], nchw_out=True)
        else:
            x = ds(x)
        return self.blocks(x)


class _CnxHead(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm = _LayerNorm2d(dim, eps=CNX_EPS)

    def forward(self, x):
        if x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled():
            return _layernorm(self.norm, x.mean(dim=(2, 3)))
        return torch.flatten(self.norm(x.mean(dim=(2, 3), keepdim=True)), 1)


class _ConvNeXtV2Backbone(nn.Module):
    """timm-shaped backbone (num_classes=0): forward(x) -> pooled, head-normalised features."""

    def __init__(self):
        super().__init__()
        self.num_features = CNX_DIMS[-1]
        self.stem = nn.Sequential(nn.Conv2d(3, CNX_DIMS[0], kernel_size=4, stride=4), _LayerNorm2d(CNX_DIMS[0], eps=CNX_EPS))
        stages, cin = [], CNX_DIMS[0]
        for i, (d, c) in enumerate(zip(CNX_DEPTHS, CNX_DIMS)):
            stages.append(_CnxStage(cin, c, d, downsample=i > 0))
            cin = c
        self.stages = nn.Sequential(*stages)
        self.head = _CnxHead(cin)
        for m in self.modules():           # timm's init: trunc_normal(std=.02) weights, zero biases
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def _stem(self, x):
        if (x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled() and x.shape[0] <= 65535 and _cfg(self).linear_three_bf16
                and x.shape[2] % 4 == 0 and x.shape[3] % 4 == 0):
            b, _, h, w = x.shape
            tok = _conv_patch_tokens(self.stem[0], x)                          # [b * h/4 * w/4, 128]
            return _layernorm(self.stem[1], tok, tokens_per_image=(h // 4) * (w // 4)).view(b, -1, h // 4, w // 4)
        return self.stem(x)

    def _forward_rows(self, x):
        """[HIP] The whole backbone with a channels-last residual stream [b * h * w, c] (no NCHW map between the patch embedding
        and the pooled head): stem = patch gather + MFMA Linear + LayerNorm rows; downsample = LayerNorm written straight into
        2 x 2 patch rows + MFMA Linear (weight in (ky, kx, c) order); blocks = _CnxBlock._forward_nhwc.
        -> (the final stream [b * h * w, c], h, w): the pre-pool map, channels-last."""
        lib = _lib.load()
        b, _, h, w = x.shape
        dev = x.device
        t = _layernorm(self.stem[1], _conv_patch_tokens(self.stem[0], x))                      # [b * h/4 * w/4, 128]
        h, w = h // 4, w // 4
        for stage in self.stages:
            ds = stage.downsample
            if isinstance(ds, nn.Sequential):
                ln, conv = ds[0], ds[1]
                pl = conv.__dict__.get("_mirx_as_linear_cl")
                if pl is None:
                    pl = _ConvAsLinear(conv, channels_last=True)
                    conv.__dict__["_mirx_as_linear_cl"] = pl
                pl.__dict__["_mirx_cfg"] = _cfg(conv)
                pl.refresh()
                c = t.shape[-1]
                rows = torch.empty((b * (h // 2) * (w // 2), 4 * c), dtype=torch.float32, device=dev)
                with torch.cuda.device(dev):
                    _lib.check(lib.mirx_layernorm_patch2_nhwc(_ptr(t), b, h, w, c, _ptr(ln.weight.detach()), _ptr(ln.bias.detach()),
                                                              float(ln.eps), _ptr(rows), _stream(dev)), "mirx_layernorm_patch2_nhwc")
                h, w = h // 2, w // 2
                t = _linear_bounded(pl, rows, _layernorm_bound(ln))
            for blk in stage.blocks:
                t = blk._forward_nhwc(t, b, h, w)
        return t, h, w

    def _forward_nhwc(self, x):
        """[HIP] _forward_rows, then the global average pool and head.norm."""
        t, h, w = self._forward_rows(x)
        pooled = t.view(x.shape[0], h * w, t.shape[-1]).mean(dim=1)                           # global average pool
        return _layernorm(self.head.norm, pooled)

    def _nhwc_ok(self, x):
        if not (x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled() and x.dim() == 4 and x.shape[0] <= 65535):
            return False
        cfg = _cfg(self)
        if not (cfg.cnx_channels_last and cfg.linear_three_bf16 and cfg.linear_two_fp16):
            return False
        h, w = x.shape[2], x.shape[3]
        if h % 32 or w % 32:                                  # stem / 4, three downsamples / 2
            return False
        return all(blk._nhwc_ok() for stage in self.stages for blk in stage.blocks)

    def forward_features(self, x):
        """timm's forward_features: the pre-pool map [b, c, h / 32, w / 32] (on the native path a channels-last view of the
        stream)."""
        if self._nhwc_ok(x):
            t, h, w = self._forward_rows(x.contiguous())
            return t.view(x.shape[0], h, w, t.shape[-1]).permute(0, 3, 1, 2)
        return self.stages(self._stem(x))

    def forward(self, x):
        if self._nhwc_ok(x):
            return self._forward_nhwc(x.contiguous())
        return self.head(self.stages(self._stem(x)))


class ConvNeXtV2(_Configurable, nn.Module):
    """Reference model.py:87-117: `convnext` backbone, optional `fc`, unit-norm output."""

    def __init__(self, pretrained=False, embedding_dim=None, weights=None):
        super().__init__()
        if pretrained and weights is None:
            raise RuntimeError("pretrained=True needs a download in the reference (model.py:96-100); "
                               "pass weights=<state dict or path> instead")
        self.convnext = _ConvNeXtV2Backbone()
        in_features = self.convnext.num_features
        self.fc = nn.Linear(in_features, embedding_dim) if embedding_dim else None
        if weights is not None:
            sd = torch.load(weights, map_location="cpu") if isinstance(weights, str) else weights
            for key in ("state-dict", "state_dict"):
                if isinstance(sd, dict) and key in sd:
                    sd = sd[key]
            self.load_state_dict(sd, strict=False)

    def forward(self, x):
        x = self.convnext(x)
        x = torch.flatten(x, 1)
        if self.fc:
            x = _linear_auto(self.fc, x)         # [HIP] three-bf16-term Linear on the inference path: no library GEMM in a forward
        if x.is_cuda and not torch.is_grad_enabled() and x.dtype == torch.float32 and x.is_contiguous():
            from .index import l2_normalize_
            return l2_normalize_(x)                # HIP F.normalize (model.py:116)
        return F.normalize(x, dim=1)


# =================================================================================================
# ConvNeXtV2 with the reference's pooling heads (model.py:120-278 there): SRA ("Spatial Residual Attention", the thesis'
# ConvNeXtV2_SRA, trained by train_sra.py) and PCAMPool (probabilistic-CAM pooling, ConvNeXtV2_PCAM).  Both heads share the
# backbone's head.norm as their `norm_layer` (one module object under two names, as there), so `convnext.*`, `sra.*` and
# `pcam.*` checkpoints load with strict=True.  On CUDA in eval mode the backbone's channels-last stream goes straight into one
# HIP head kernel (k_attnpool.hip); everywhere else the heads below are the reference's formulas in torch.
# =================================================================================================
ATTNPOOL_MAX_C = 8192             # include/mirx.h: the limits mirx_sra_head_nhwc / mirx_pcam_head_nhwc accept
ATTNPOOL_MAX_K = 64
ATTNPOOL_LDS_FLOATS = 16384       # (K + 3) * hw <= this


def _attnpool_ok(c, k, hw):
    return c % 4 == 0 and 4 <= c <= ATTNPOOL_MAX_C and 1 <= k <= ATTNPOOL_MAX_K and hw >= 1 and (k + 3) * hw <= ATTNPOOL_LDS_FLOATS


def _load_local_weights(model, weights):
    """ConvNeXtV2's rules: a state dict or a path to one (optionally under "state-dict" / "state_dict"), loaded strict=False."""
    sd = torch.load(weights, map_location="cpu") if isinstance(weights, str) else weights
    for key in ("state-dict", "state_dict"):
        if isinstance(sd, dict) and key in sd:
            sd = sd[key]
    model.load_state_dict(sd, strict=False)


class SRA(nn.Module):
    """Reference model.py:120-164: GAP + LayerNorm plus lam x the LayerNormed mean over K softmax-attention pools."""

    def __init__(self, input_dim, num_heads=8, lam=0.1, norm_layer=None):
        super().__init__()
        self.num_heads = num_heads
        self.lam = lam
        self.norm_layer = norm_layer
        self.conv_att = nn.Conv2d(input_dim, num_heads, kernel_size=1, bias=False)
        self.softmax = nn.Softmax(dim=2)
        nn.init.normal_(self.conv_att.weight, mean=0.0, std=1e-4)

    def forward(self, x):
        b, c, h, w = x.shape
        gap = x.mean(dim=(2, 3), keepdim=True)
        if self.norm_layer is not None:
            gap = self.norm_layer(gap)
        gap = torch.flatten(gap, 1)
        att = self.softmax(self.conv_att(x).reshape(b, self.num_heads, h * w))          # [b, K, hw]
        pooled = torch.bmm(att, x.reshape(b, c, h * w).permute(0, 2, 1)).mean(dim=1).reshape(b, c, 1, 1)
        if self.norm_layer is not None:
            pooled = self.norm_layer(pooled)
        return gap + self.lam * torch.flatten(pooled, 1)


class PCAMPool(nn.Module):
    """Reference model.py:199-257: probabilistic-CAM pooling -> (embedding, class_logits, pcam_probs)."""

    def __init__(self, input_dim, num_classes, lam=0.1, norm_layer=None, embedding_dim=None):
        super().__init__()
        self.num_classes = num_classes
        self.lam = lam
        self.norm_layer = norm_layer
        self.classifier = nn.Conv2d(input_dim, num_classes, kernel_size=1)
        self.fc = nn.Linear(input_dim, embedding_dim) if embedding_dim else None

    def forward(self, x):
        b, c, h, w = x.shape
        gap = x.mean(dim=(2, 3), keepdim=True)
        if self.norm_layer is not None:
            gap = self.norm_layer(gap)
        gap = torch.flatten(gap, 1)
        z = self.norm_layer(x) if self.norm_layer is not None else x
        probs = torch.sigmoid(self.classifier(z))                                         # [b, K, h, w]
        q = probs.reshape(b, self.num_classes, h * w)
        q = q / (q.sum(dim=2, keepdim=True) + 1e-8)
        pooled = torch.bmm(q, z.reshape(b, c, h * w).permute(0, 2, 1))                    # [b, K, c]
        logits = torch.einsum("bkc,kc->bk", pooled, self.classifier.weight.reshape(self.num_classes, c))
        if self.classifier.bias is not None:
            logits = logits + self.classifier.bias
        feat = gap + self.lam * (F.softmax(logits, dim=1).unsqueeze(2) * pooled).sum(dim=1)
        if self.fc is not None:
            feat = self.fc(feat)
        return F.normalize(feat, dim=1), logits, probs


def _native_head_ok(model, x, k):
    """The backbone's native path takes x, the model is in eval mode, and the head kernel's limits hold for the final map."""
    bb = model.convnext
    if model.training or not bb._nhwc_ok(x):
        return False
    return _attnpool_ok(bb.num_features, k, (x.shape[2] // 32) * (x.shape[3] // 32))


def _head_rows(model, x):
    """[HIP] The backbone's final channels-last stream and the head norm's arguments."""
    t, h, w = model.convnext._forward_rows(x.contiguous())
    ln = model.convnext.head.norm
    return t, h * w, t.shape[-1], _ptr(ln.weight.detach()), _ptr(ln.bias.detach()), float(ln.eps)


class ConvNeXtV2_SRA(_Configurable, nn.Module):
    """Reference model.py:167-196: `convnext` backbone + `sra` head (norm_layer = convnext.head.norm), unit-norm [B, 1024]."""

    def __init__(self, pretrained=False, num_heads=8, lam=0.1, weights=None):
        super().__init__()
        if pretrained and weights is None:
            raise RuntimeError("pretrained=True needs a download in the reference (model.py:176-180); "
                               "pass weights=<state dict or path> instead")
        self.convnext = _ConvNeXtV2Backbone()
        self.sra = SRA(self.convnext.num_features, num_heads=num_heads, lam=lam, norm_layer=self.convnext.head.norm)
        if weights is not None:
            _load_local_weights(self, weights)

    def forward(self, x):
        if _native_head_ok(self, x, self.sra.num_heads):
            t, hw, c, g, bt, eps = _head_rows(self, x)
            wa = self.sra.conv_att.weight.detach().reshape(self.sra.num_heads, c)
            y = torch.empty((x.shape[0], c), dtype=torch.float32, device=x.device)
            with torch.cuda.device(x.device):
                _lib.check(_lib.load().mirx_sra_head_nhwc(_ptr(t), x.shape[0], hw, c, _ptr(wa), self.sra.num_heads, g, bt, eps,
                                                          float(self.sra.lam), 1, _ptr(y), _stream(x.device)), "mirx_sra_head_nhwc")
            return y
        return F.normalize(self.sra(self.convnext.forward_features(x)), dim=1)


class ConvNeXtV2_PCAM(_Configurable, nn.Module):
    """Reference model.py:260-278: `convnext` backbone + `pcam` head; eval -> unit-norm [B, embedding_dim or 1024], training ->
    {"embedding", "class_logits", "pcam_maps"}."""

    def __init__(self, pretrained=False, num_classes=3, lam=0.1, embedding_dim=None, weights=None):
        super().__init__()
        if pretrained and weights is None:
            raise RuntimeError("pretrained=True needs a download in the reference (model.py:263-267); "
                               "pass weights=<state dict or path> instead")
        self.convnext = _ConvNeXtV2Backbone()
        self.pcam = PCAMPool(self.convnext.num_features, num_classes=num_classes, lam=lam, norm_layer=self.convnext.head.norm,
                             embedding_dim=embedding_dim)
        if weights is not None:
            _load_local_weights(self, weights)

    def forward(self, x):
        pc = self.pcam
        if pc.classifier.bias is not None and _native_head_ok(self, x, pc.num_classes):
            t, hw, c, g, bt, eps = _head_rows(self, x)
            wc = pc.classifier.weight.detach().reshape(pc.num_classes, c)
            feat = torch.empty((x.shape[0], c), dtype=torch.float32, device=x.device)
            with torch.cuda.device(x.device):
                _lib.check(_lib.load().mirx_pcam_head_nhwc(_ptr(t), x.shape[0], hw, c, _ptr(wc), _ptr(pc.classifier.bias.detach()),
                                                           pc.num_classes, g, bt, eps, float(pc.lam), int(pc.fc is None),
                                                           _ptr(feat), None, _stream(x.device)), "mirx_pcam_head_nhwc")
            if pc.fc is None:
                return feat
            return _normalize_rows(_linear_auto(pc.fc, feat))
        embedding, class_logits, probs = pc(self.convnext.forward_features(x))
        if self.training:
            return {"embedding": embedding, "class_logits": class_logits, "pcam_maps": probs}
        return embedding

# =================================================================================================
# DINOv2 ViT-B/14 (reference model.py:448-494 and nih_multilabel_retrieval.py:170-221 around timm
# 'vit_base_patch14_dinov2.lvd142m', num_classes=0).  Module tree reproduces timm's parameter names
# (cls_token, pos_embed, patch_embed.proj, blocks.N.{norm1,attn.qkv,attn.proj,ls1.gamma,norm2,
# mlp.fc1,mlp.fc2,ls2.gamma}, norm) so `backbone.*` checkpoints load unchanged.
# =================================================================================================
class _LayerScale(nn.Module):
    def __init__(self, dim, init=1e-5):
        super().__init__()
        self.gamma = nn.Parameter(init * torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class _VitAttention(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.num_heads = heads
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        b, n, c = x.shape
        dh = c // self.num_heads
        qkv = self.qkv(x)                                                # [b, n, 3, heads, dh] packed
        if x.is_cuda and dh in (32, 64, 72, 96) and qkv.dtype == torch.float32 and not torch.is_grad_enabled():
            # MI355X inference path: flash attention straight on the packed projection, output already [b, n, heads * dh]
            # (the rocBLAS projection gives no bounds: three bf16 terms, or fp32 MFMAs when the configuration says so)
            inf = float("inf")
            return self.proj(_attention_packed(self, qkv.contiguous(), self.num_heads, dh, float(dh) ** -0.5, inf, inf,
                                               fp32_fallback=True)[0])
        qkv = qkv.reshape(b, n, 3, self.num_heads, dh).permute(2, 0, 3, 1, 4)
        a = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2])      # softmax(q k^T / sqrt(d)) v
        return self.proj(a.transpose(1, 2).reshape(b, n, c))


class _VitMlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class _VitBlock(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _VitAttention(dim, heads)
        self.ls1 = _LayerScale(dim)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _VitMlp(dim, 4 * dim)
        self.ls2 = _LayerScale(dim)

    def forward(self, x):
        at = self.attn
        if (x.dim() == 3 and x.shape[-1] // at.num_heads == 64 and _linear_s3_ok(at.qkv, x)
                and _linear_s3_ok(at.proj, x) and _linear_s3_ok(self.mlp.fc1, x) and _linear_s3_ok(self.mlp.fc2, x)):
            c = x.shape[-1]
            return _prenorm_block(self, x, self.norm1, at.qkv, at.proj, self.norm2, self.mlp.fc1, self.mlp.fc2, at.num_heads, 64, 0.125,
                                  bqk=_linear_out_bound(self.norm1, at.qkv, slice(0, 2 * c)),
                                  bv=_linear_out_bound(self.norm1, at.qkv, slice(2 * c, 3 * c)),
                                  bh=_linear_out_bound(self.norm2, self.mlp.fc1), gelu=1, gamma1=self.ls1.gamma,
                                  gamma2=self.ls2.gamma, fp32_fallback=True)
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


class _PatchEmbed(nn.Module):
    def __init__(self, dim, patch):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=patch, stride=patch)

    def forward(self, x):
        if x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled() and x.shape[0] <= 65535 and _cfg(self).linear_three_bf16:
            # MI355X path: the stride-14 patch convolution as patch gather + MFMA Linear (no library convolution)
            return _conv_patch_tokens(self.proj, x).view(x.shape[0], -1, self.proj.out_channels)
        return self.proj(x).flatten(2).transpose(1, 2)


class _Dinov2Backbone(nn.Module):
    """timm VisionTransformer surface used by the reference: forward(x) -> CLS feature [B,C],
    forward_features(x) -> tokens [B,1+N,C], .blocks, .norm, .num_features."""

    def __init__(self, img_size=518, patch=14, dim=768, depth=12, heads=12):
        super().__init__()
        self.num_features = dim
        self.patch_size = patch
        self.grid = img_size // patch
        self.patch_embed = _PatchEmbed(dim, patch)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(0.02 * torch.randn(1, 1 + self.grid * self.grid, dim))
        self.blocks = nn.Sequential(*[_VitBlock(dim, heads) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        nn.init.normal_(self.cls_token, std=1e-6)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def _pos(self, gh, gw):
        if gh == self.grid and gw == self.grid:
            return self.pos_embed
        # other input sizes: bicubic resampling of the patch grid (timm resample_abs_pos_embed)
        cls, grid = self.pos_embed[:, :1], self.pos_embed[:, 1:]
        grid = grid.reshape(1, self.grid, self.grid, -1).permute(0, 3, 1, 2)
        grid = F.interpolate(grid, size=(gh, gw), mode="bicubic", antialias=True, align_corners=False)
        return torch.cat([cls, grid.permute(0, 2, 3, 1).reshape(1, gh * gw, -1)], dim=1)

    def forward_features(self, x):
        gh, gw = x.shape[-2] // self.patch_size, x.shape[-1] // self.patch_size
        x = self.patch_embed(x)
        x = torch.cat([self.cls_token.expand(x.shape[0], -1, -1), x], dim=1) + self._pos(gh, gw)
        return _layernorm(self.norm, self.blocks(x))

    def forward(self, x):
        return self.forward_features(x)[:, 0]


def _normalize_rows(x):
    if x.is_cuda and not torch.is_grad_enabled() and x.dtype == torch.float32:
        from .index import l2_normalize_
        return l2_normalize_(x.contiguous().clone())
    return F.normalize(x, dim=1)


class DinoV2(_Configurable, nn.Module):
    """Reference model.py:448-494 (`backbone`, `fc`; the last `unfreeze_blocks` blocks + final norm
    trainable, the rest frozen)."""

    def __init__(self, model_name="vit_base_patch14_dinov2.lvd142m", pretrained=False, embedding_dim=None,
                 unfreeze_blocks=3, weights=None, img_size=518):
        super().__init__()
        if pretrained and weights is None:
            raise RuntimeError("pretrained=True needs a download in the reference (model.py:459-463); "
                               "pass weights=<state dict or path> instead")
        if model_name != "vit_base_patch14_dinov2.lvd142m":
            raise ValueError(f"Unknown DINOv2 backbone: {model_name}")
        self.backbone = _Dinov2Backbone(img_size=img_size)
        for p in self.backbone.parameters():
            p.requires_grad = False
        nb = max(0, min(unfreeze_blocks, len(self.backbone.blocks)))
        if nb > 0:
            for blk in list(self.backbone.blocks)[-nb:]:
                for p in blk.parameters():
                    p.requires_grad = True
        for p in self.backbone.norm.parameters():
            p.requires_grad = True
        self.fc = nn.Linear(self.backbone.num_features, embedding_dim) if embedding_dim else None
        if weights is not None:
            sd = torch.load(weights, map_location="cpu") if isinstance(weights, str) else weights
            for key in ("state-dict", "state_dict"):
                if isinstance(sd, dict) and key in sd:
                    sd = sd[key]
            self.load_state_dict(sd, strict=False)

    def forward(self, x):
        x = torch.flatten(self.backbone(x), 1)
        if self.fc:
            x = _linear_auto(self.fc, x)         # [HIP] three-bf16-term Linear on the inference path: no library GEMM in a forward
        return _normalize_rows(x)


class DINOv2MultiLabelRetrievalModel(_Configurable, nn.Module):
    """Reference nih_multilabel_retrieval.py:170-221: dict with cls_embedding / projection /
    embedding (unit norm, 256-d) / logits."""

    def __init__(self, num_labels=14, backbone_name="vit_base_patch14_dinov2.lvd142m", pretrained=False, img_size=518):
        super().__init__()
        if pretrained:
            raise RuntimeError("pretrained=True needs a download in the reference; load a state dict instead")
        if backbone_name != "vit_base_patch14_dinov2.lvd142m":
            raise ValueError(f"Unknown DINOv2 backbone: {backbone_name}")
        self.backbone = _Dinov2Backbone(img_size=img_size)
        self.projection_head = nn.Sequential(nn.Linear(self.backbone.num_features, 512), nn.GELU(), nn.Linear(512, 256))
        self.classification_head = nn.Linear(256, num_labels)

    def forward(self, images):
        cls_embedding = self.backbone.forward_features(images)[:, 0]
        projection = self.projection_head(cls_embedding)
        return {"cls_embedding": cls_embedding, "projection": projection,
                "embedding": _normalize_rows(projection), "logits": self.classification_head(projection)}


class ConvNeXtV2MultiLabelRetrievalModel(_Configurable, nn.Module):
    """Reference nih_multilabel_retrieval.py:224-257."""

    def __init__(self, num_labels=14, backbone_name="convnextv2_base.fcmae_ft_in22k_in1k_384", pretrained=False):
        super().__init__()
        if pretrained:
            raise RuntimeError("pretrained=True needs a download in the reference; load a state dict instead")
        self.backbone = _ConvNeXtV2Backbone()
        self.projection_head = nn.Sequential(nn.Linear(self.backbone.num_features, 512), nn.GELU(), nn.Linear(512, 256))
        self.classification_head = nn.Linear(256, num_labels)

    def forward(self, images):
        features = self.backbone(images)
        projection = self.projection_head(features)
        return {"backbone_embedding": features, "projection": projection,
                "embedding": _normalize_rows(projection), "logits": self.classification_head(projection)}


# =================================================================================================
# MedSigLIP (reference model.py:536-634): SigLIP so400m vision tower -> pooler_output ->
# Linear(h,512)-LayerNorm-ReLU-Linear(512,embed_dim) -> L2 normalise.  The reference takes the tower
# from `AutoModel.from_pretrained("google/medsiglip-448").vision_model` (a download); here the same
# transformers class is built from a LOCAL config, so `backbone.*` / `projection.*` checkpoints
# load unchanged and nothing is fetched.
# =================================================================================================
class MedSigLIP(_Configurable, nn.Module):
    """Reference model.py:536-634: `backbone` (the SigLIP vision tower), `projection`, unit-norm output."""

    def __init__(self, model_name="google/medsiglip-448", embed_dim=512, unfreeze_layers=2, vision_config=None,
                 weights=None):
        super().__init__()
        from .siglip import MEDSIGLIP_VISION, SiglipVisionTower
        self.backbone = SiglipVisionTower(**(vision_config or MEDSIGLIP_VISION))
        for p in self.backbone.parameters():
            p.requires_grad = False
        if unfreeze_layers > 0:
            for layer in self.backbone.encoder.layers[-unfreeze_layers:]:
                for p in layer.parameters():
                    p.requires_grad = True
            for p in self.backbone.post_layernorm.parameters():
                p.requires_grad = True
        hidden = self.backbone.config.hidden_size
        self.projection = nn.Sequential(nn.Linear(hidden, 512), nn.LayerNorm(512), nn.ReLU(), nn.Linear(512, embed_dim))
        if weights is not None:
            sd = torch.load(weights, map_location="cpu") if isinstance(weights, str) else weights
            for key in ("state-dict", "state_dict"):
                if isinstance(sd, dict) and key in sd:
                    sd = sd[key]
            self.load_state_dict(sd, strict=False)

    def ensure_eager_attention(self):
        """Kept for callers (milvus_retrieval.py:172); attention maps always come from the explicit softmax path."""
        self.backbone.config._attn_implementation = "eager"

    def verify_attention_output(self, device="cuda"):
        self.eval()
        size = self.backbone.config.image_size
        with torch.no_grad():
            out = self.backbone(pixel_values=torch.randn(1, 3, size, size, device=device), output_attentions=True,
                                return_dict=True)
        return out.attentions is not None and len(out.attentions) > 0 and out.attentions[0].numel() > 0

    def forward(self, x):
        features = self.backbone(pixel_values=x).pooler_output
        p = self.projection
        h = torch.relu(_layernorm(p[1], _linear_auto(p[0], features)))
        return _normalize_rows(_linear_auto(p[3], h))


# =================================================================================================
# ResNet-50 (reference model.py:9-39: torchvision resnet50 without its classifier, children [:-1]).  torchvision is not a
# dependency: the tree below reproduces its names -- resnet50 = Sequential(conv1, bn1, relu, maxpool, layer1..layer4, avgpool)
# with indices 0-8, Bottleneck blocks {conv1, bn1, conv2, bn2, conv3, bn3, relu, downsample.0/.1}, the stride on conv2
# (v1.5) -- so reference checkpoints (`resnet50.*`, `fc.*`) load unchanged.  23 508 032 backbone parameters.
#
# MI355X path (CUDA input, eval mode, grad off): the stem is DenseNet's (conv 7x7 / 2 + BN + ReLU + max-pool, one kernel,
# mirx_stem_conv7_bn_relu_pool_split2h_into / _u8_into), turned into channels-last terms rows by one glue pass; every other
# convolution is mirx_conv_terms (k_conv_t2.hip) with its BatchNorm folded, the block's residual and ReLU in the epilogue;
# the head is mirx_gap_nhwc_l2norm on the last block's fp32 rows; fc through _linear_auto.  DESIGN 15.
# =================================================================================================
RESNET_LAYERS = (3, 4, 6, 3)
RESNET_WIDTHS = (64, 128, 256, 512)


class _Bottleneck(nn.Module):
    """torchvision Bottleneck (expansion 4, stride on the 3x3 convolution)."""
    expansion = 4

    def __init__(self, cin, width, stride):
        super().__init__()
        cout = width * self.expansion
        self.conv1 = nn.Conv2d(cin, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = (nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride, bias=False), nn.BatchNorm2d(cout))
                           if stride != 1 or cin != cout else None)
        self.stride = stride

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.relu(self.bn2(self.conv2(y)))
        return self.relu(self.bn3(self.conv3(y)) + idt)


def _make_resnet50():
    mods = [nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
            nn.MaxPool2d(3, stride=2, padding=1)]
    cin = 64
    for i, (nb, width) in enumerate(zip(RESNET_LAYERS, RESNET_WIDTHS)):
        blocks = []
        for j in range(nb):
            blocks.append(_Bottleneck(cin, width, 2 if (i > 0 and j == 0) else 1))
            cin = width * _Bottleneck.expansion
        mods.append(nn.Sequential(*blocks))
    mods.append(nn.AdaptiveAvgPool2d((1, 1)))
    seq = nn.Sequential(*mods)
    for m in seq.modules():                                # torchvision's initialisation
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
    return seq, cin


def _conv_terms_weights(conv, bn):
    """A convolution with its eval BatchNorm folded, as mirx_conv_terms takes it: dict of wt (terms rows of W[o] * ws[o] in K
    order (ky, kx, c), rows padded to a multiple of 128), oscale = 1 / ws, bias, and the host constants of the output bound
    (w_abs_sum = max_o sum |W[o, :]|, bias_abs_max = max |bias|), plus the geometry."""
    scale, shift = _bn_affine(bn)
    w = conv.weight.detach().float() * scale.view(-1, 1, 1, 1)
    cout, cin, k, _ = w.shape
    wk = w.permute(0, 2, 3, 1).reshape(cout, k * k * cin)
    ws = _pow2_row_scales(wk)
    wp = wk * ws[:, None]
    if cout % 128:
        wp = F.pad(wp, (0, 0, 0, 128 - cout % 128))
    return {"wt": _terms_of(wp, 1.0), "osc": (1.0 / ws).contiguous(), "bias": shift.contiguous(),
            "wsum": float(wk.abs().sum(dim=1).max()), "bmax": float(shift.abs().max()),
            "k": k, "s": conv.stride[0], "cin": cin, "cout": cout}


def _out_side(side, k, s):
    p = (k - 1) // 2
    return (side + 2 * p - k) // s + 1


def conv_terms(cw, x, h, w, res=None, relu=True, terms_out=True, fp32_out=False, out_range=None):
    """[HIP] one mirx_conv_terms launch.  cw = _conv_terms_weights(..); x = (terms rows fp16 [n * h * w, 2 cin], scale row [n],
    range row [n]); res = (terms rows, scale row, range row) of the residual or None.  -> (yt, y_scale, y_range, y_fp32, ho, wo)
    with yt / y_scale None unless terms_out and y_fp32 None unless fp32_out; out_range: the range row to fold max |y| into
    (zeroed by the caller; a fresh one by default)."""
    xt, xs, xr = x
    n = xs.shape[0]
    ho, wo = _out_side(h, cw["k"], cw["s"]), _out_side(w, cw["k"], cw["s"])
    dev = xt.device
    m = n * ho * wo
    yt = torch.empty((m, 2 * cw["cout"]), dtype=torch.float16, device=dev) if terms_out else None
    ys = torch.empty((n,), dtype=torch.float32, device=dev) if terms_out else None
    y = torch.empty((m, cw["cout"]), dtype=torch.float32, device=dev) if fp32_out else None
    yr = torch.zeros((n,), dtype=torch.float32, device=dev) if out_range is None else out_range
    rt, rs, rr = res if res is not None else (None, None, None)
    p = lambda t: None if t is None else _ptr(t)          # noqa: E731
    _lib.check(_lib.load().mirx_conv_terms(_ptr(xt), _ptr(xs), _ptr(xr), n, h, w, cw["cin"], cw["k"], cw["s"], _ptr(cw["wt"]),
                                           _ptr(cw["osc"]), _ptr(cw["bias"]), cw["cout"], cw["wsum"], cw["bmax"], p(rt), p(rs),
                                           p(rr), 1 if relu else 0, p(yt), p(ys), p(y), _ptr(yr), _stream(dev)),
               "mirx_conv_terms")
    return yt, ys, yr, y, ho, wo


class ResNet50(_Configurable, _InferenceCache, nn.Module):
    """Reference model.py:9-39 (ResNet50), MI355X-native inference path."""
    accepts_uint8 = True        # forward() takes raw 8-bit images and applies ToTensor + Normalize itself (input_mean / input_std)

    def __init__(self, pretrained=False, embedding_dim=None, num_labels=None, weights=None):
        super().__init__()
        if pretrained and weights is None:
            raise RuntimeError("pretrained=True needs a download in the reference (model.py:13); "
                               "pass weights=<state dict or path> instead")
        self.resnet50, in_features = _make_resnet50()
        self.fc = nn.Linear(in_features, embedding_dim) if embedding_dim else None
        out_features = embedding_dim if embedding_dim else in_features
        self.classification_head = nn.Linear(out_features, num_labels) if num_labels else None
        self.register_buffer("input_mean", torch.tensor(IMAGENET_MEAN, dtype=torch.float32), persistent=False)
        self.register_buffer("input_std", torch.tensor(IMAGENET_STD, dtype=torch.float32), persistent=False)
        self._infer_cache = None
        self._init_config()
        if weights is not None:
            sd = torch.load(weights, map_location="cpu") if isinstance(weights, str) else weights
            for key in ("state-dict", "state_dict"):
                if isinstance(sd, dict) and key in sd:
                    sd = sd[key]
            self.load_state_dict(sd, strict=False)

    # -- the plain module graph (training, CPU tensors): same ops as the reference -------------
    def forward_eager(self, x):
        return torch.flatten(self.resnet50(x), 1)

    def normalize_uint8(self, x):
        """ToTensor + Normalize of the reference (test.py:1309-1332) on uint8 [B, 3, H, W]: what the stem kernel's table holds."""
        m = self.input_mean.to(x.device).view(1, 3, 1, 1)
        s_ = self.input_std.to(x.device).view(1, 3, 1, 1)
        return (x.float() / 255.0 - m) / s_

    # -- MI355X inference path -------------------------------------------------------------------
    def _watch_root(self):
        return self.resnet50

    def _blocks(self):
        return [blk for layer in self.resnet50[4:8] for blk in layer]

    def _prepare_inference(self):
        """Fold every eval-mode BatchNorm into its convolution and pre-split the weights, once per weight version."""
        r = self.resnet50
        cache = {"stem": _stem_weights_split2h(r[0].weight) + _bn_affine(r[1]), "blocks": []}
        for blk in self._blocks():
            e = {"conv1": _conv_terms_weights(blk.conv1, blk.bn1), "conv2": _conv_terms_weights(blk.conv2, blk.bn2),
                 "conv3": _conv_terms_weights(blk.conv3, blk.bn3)}
            if blk.downsample is not None:
                e["down"] = _conv_terms_weights(blk.downsample[0], blk.downsample[1])
            cache["blocks"].append(e)
        cache["_cuda"] = r[0].weight.is_cuda
        self._infer_cache = cache
        self._mark_built(cache)
        return cache

    def _features_native(self, x, cache):
        """-> fp32 rows [B * h/32 * w/32, 2048] of layer4's output (channels last) and the pixels per image."""
        out, side_h, side_w = self._features_native_sides(x, cache)
        return out, side_h * side_w

    def _features_native_sides(self, x, cache):
        """-> fp32 rows [B * h/32 * w/32, 2048] of layer4's output (channels last) and its height and width."""
        lib = _lib.load()
        u8 = x.dtype == torch.uint8
        x = x.contiguous() if u8 else x.contiguous().float()
        b, _, h, w = x.shape
        dev = x.device
        st = _stream(dev)
        blocks = cache["blocks"]
        # range rows: the input images, the stem's output, then per block conv1 / conv2 / downsample / conv3
        ranges = torch.zeros((2 + 4 * len(blocks), b), dtype=torch.float32, device=dev)
        xr = ranges[0]
        if u8:
            _lib.check(lib.mirx_range_absmax_u8(_ptr(x), h * w, b, _ptr(self.input_mean), _ptr(self.input_std), _ptr(xr), st),
                       "mirx_range_absmax_u8")
        else:
            _lib.check(lib.mirx_range_absmax(_ptr(x), x[0].numel(), b, _ptr(xr), st), "mirx_range_absmax")
        w2, osc, sc, sh = cache["stem"]
        hs, wsd = h // 4, w // 4
        y0 = torch.empty((b, 64, hs, wsd), dtype=torch.float32, device=dev)
        if u8:
            _lib.check(lib.mirx_stem_conv7_bn_relu_pool_split2h_u8_into(_ptr(x), _ptr(self.input_mean), _ptr(self.input_std),
                                                                        _ptr(w2), _ptr(osc), _ptr(sc), _ptr(sh), b, h, w,
                                                                        _ptr(y0), 64 * hs * wsd, _ptr(xr), _ptr(ranges[1]), st),
                       "mirx_stem_split2h_u8_into")
        else:
            _lib.check(lib.mirx_stem_conv7_bn_relu_pool_split2h_into(_ptr(x), _ptr(w2), _ptr(osc), _ptr(sc), _ptr(sh), b, h, w,
                                                                     _ptr(y0), 64 * hs * wsd, _ptr(xr), _ptr(ranges[1]), st),
                       "mirx_stem_split2h_into")
        t0 = torch.empty((b * hs * wsd, 128), dtype=torch.float16, device=dev)
        s0 = torch.empty((b,), dtype=torch.float32, device=dev)
        _lib.check(lib.mirx_nchw_to_terms(_ptr(y0), 64 * hs * wsd, b, 64, hs * wsd, _ptr(ranges[1]), _ptr(s0), _ptr(t0), st),
                   "mirx_nchw_to_terms")
        del y0
        cur, side_h, side_w = (t0, s0, ranges[1]), hs, wsd
        out = None
        for i, e in enumerate(blocks):
            last = i == len(blocks) - 1
            r = 2 + 4 * i
            t1, s1, r1, _, h1, w1 = conv_terms(e["conv1"], cur, side_h, side_w, out_range=ranges[r])
            t2, s2, r2, _, h2, w2 = conv_terms(e["conv2"], (t1, s1, r1), h1, w1, out_range=ranges[r + 1])
            del t1
            if "down" in e:
                td, sd_, rd, _, _, _ = conv_terms(e["down"], cur, side_h, side_w, relu=False, out_range=ranges[r + 2])
                res = (td, sd_, rd)
            else:
                res = cur
            t3, s3, r3, out, h3, w3 = conv_terms(e["conv3"], (t2, s2, r2), h2, w2, res=res, terms_out=not last,
                                                 fp32_out=last, out_range=ranges[r + 3])
            cur, side_h, side_w = (t3, s3, r3), h3, w3
        self.__dict__["_mirx_last_ranges"] = ranges                 # kept for diagnostics (the bound's bit cost)
        return out, side_h, side_w

    @staticmethod
    def _native_size_ok(x):
        return x.shape[-1] % 4 == 0 and x.shape[-2] % 4 == 0 and x.shape[-1] >= 8 and x.shape[-2] >= 8

    def _layer4_rows(self, x, cache):
        """[HIP] the output of resnet50[7][-1] as fp32 channels-last rows [B, h * w, 2048] -> (rows, h, w): SimCAM's tap."""
        rows, h, w = self._features_native_sides(x, cache)
        return rows.view(x.shape[0], h * w, rows.shape[-1]), h, w

    def _embed_native(self, x, normalize, cache):
        b, _, h, w = x.shape
        if not self._native_size_ok(x):
            raise ValueError(f"ResNet50 native path: H and W must be multiples of 4 and at least 8 (got {h} x {w}); "
                             f"resize the input (the reference's transform gives 224 x 224)")
        if b > 65535:
            return torch.cat([self._embed_native(x[i:i + 65535], normalize, cache) for i in range(0, b, 65535)])
        rows, hw = self._features_native(x, cache)
        out = torch.empty((b, rows.shape[1]), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().mirx_gap_nhwc_l2norm(_ptr(rows), b, hw, rows.shape[1], 1 if normalize else 0, _ptr(out),
                                                    _stream(x.device)), "mirx_gap_nhwc_l2norm")
        return out

    def forward(self, x):
        native = x.is_cuda and not self.training and not torch.is_grad_enabled()
        if native:
            with torch.cuda.device(x.device):
                cache = self._cache()
                plain_head = self.fc is None and self.classification_head is None
                x = self._embed_native(x, plain_head, cache)
                if plain_head:
                    return x                       # already unit-norm (reference model.py:38)
        else:
            x = self.forward_eager(self.normalize_uint8(x) if x.dtype == torch.uint8 else x)
        if self.fc:
            x = _linear_auto(self.fc, x)         # [HIP] on the inference path: no library GEMM in a forward
        if self.classification_head is not None:
            return {"embedding": F.normalize(x, dim=1), "logits": self.classification_head(x)}
        return F.normalize(x, dim=1)


# =================================================================================================
# SwinV2-B (reference model.py:418-446: timm 0.9.7 `swinv2_base_window12to24_192to384.ms_in22k_ft_in1k`, num_classes=0, at
# 384 x 384, + optional fc + F.normalize).  timm is not a dependency: the tree below reproduces its names -- swinv2.patch_embed.
# {proj, norm}, swinv2.layers.{0..3}.{downsample (PatchMerging at the START of stages 1-3), blocks.j.{attn.{qkv, q_bias, v_bias,
# logit_scale, cpb_mlp.{0,2}, proj}, norm1, mlp.{fc1, fc2}, norm2}}, swinv2.norm -- so reference checkpoints load unchanged.
# k_bias, relative_coords_table, relative_position_index and attn_mask are derived from the configuration (non-persistent; a
# checkpoint that carries them loads and is not read).  86 893 816 backbone parameters.  Res-post-norm blocks:
#   x = x + norm1(attn(x)),  x = x + norm2(mlp(x)).
#
# MI355X path (CUDA fp32 384 x 384 input, eval mode, grad off), per block: qkv Linear (mirx_linear_terms) -> shifted-window
# cosine attention written as terms rows (mirx_window_attention_split2h: roll / partition / mask by addressing, compact bias
# table) -> proj -> x += norm1(.) with x also written as terms rows (mirx_swin_postnorm) -> fc1 + GELU as terms -> fc2 ->
# x += norm2(.).  Stages start with mirx_patch_merge_terms -> reduction -> LayerNorm; the stem is _conv_patch_tokens; the head
# the final LayerNorm + mirx_gap_nhwc_l2norm.  Every Linear reads two fp16 terms scaled by a host-side bound of its input
# (the residual stream's bound grows by the LayerNorm bounds of norm1 / norm2 per block).  DESIGN 16.
# =================================================================================================
SWIN_IMG = 384
SWIN_PATCH = 4
SWIN_DEPTHS = (2, 2, 18, 2)
SWIN_DIMS = (128, 256, 512, 1024)
SWIN_HEADS = (4, 8, 16, 32)
SWIN_WINDOW = 24
SWIN_PRETRAINED_WINDOWS = (12, 12, 12, 6)
SWIN_CHUNK = 64                 # images per pass of the native path (bounds the activation memory; results do not depend on it)
_SWIN_DERIVED = ("k_bias", "relative_coords_table", "relative_position_index")


class _SwinAttention(nn.Module):
    """timm 0.9.7 swin_transformer_v2.WindowAttention: cosine attention with a learned per-head logit scale and a continuous
    relative-position bias (cpb_mlp over a log-spaced coordinate table)."""

    def __init__(self, dim, heads, window, pretrained_window):
        super().__init__()
        self.dim, self.num_heads, self.window = dim, heads, window
        self.logit_scale = nn.Parameter(torch.log(10 * torch.ones((heads, 1, 1))))
        self.cpb_mlp = nn.Sequential(nn.Linear(2, 512, bias=True), nn.ReLU(inplace=True), nn.Linear(512, heads, bias=False))
        r = torch.arange(-(window - 1), window, dtype=torch.float32)
        table = torch.stack(torch.meshgrid([r, r], indexing="ij")).permute(1, 2, 0).contiguous().unsqueeze(0)
        table /= (pretrained_window - 1) if pretrained_window > 0 else (window - 1)
        table *= 8
        table = torch.sign(table) * torch.log2(torch.abs(table) + 1.0) / math.log2(8)
        self.register_buffer("relative_coords_table", table, persistent=False)          # [1, 2w-1, 2w-1, 2]
        c = torch.arange(window)
        coords = torch.stack(torch.meshgrid([c, c], indexing="ij")).flatten(1)          # [2, w*w]
        rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0)
        self.register_buffer("relative_position_index", (rel[..., 0] + window - 1) * (2 * window - 1) + rel[..., 1] + window - 1,
                             persistent=False)                                            # [w*w, w*w]
        self.qkv = nn.Linear(dim, dim * 3, bias=False)
        self.q_bias = nn.Parameter(torch.zeros(dim))
        self.register_buffer("k_bias", torch.zeros(dim), persistent=False)
        self.v_bias = nn.Parameter(torch.zeros(dim))
        self.proj = nn.Linear(dim, dim)

    def _load_from_state_dict(self, state_dict, prefix, *a, **k):
        for name in _SWIN_DERIVED:                     # derived from the configuration: a checkpoint's copy is not read
            state_dict.pop(prefix + name, None)
        return super()._load_from_state_dict(state_dict, prefix, *a, **k)

    def bias_table(self):
        """16 sigmoid(cpb_mlp(relative_coords_table)) -> [heads, (2 w - 1)^2] (the compact table the kernel gathers from)."""
        t = self.cpb_mlp(self.relative_coords_table.to(self.cpb_mlp[0].weight.dtype)).view(-1, self.num_heads)
        return (16 * torch.sigmoid(t)).t()

    def logit_scales(self):
        return torch.clamp(self.logit_scale, max=math.log(1.0 / 0.01)).exp()

    def forward(self, x, mask=None):
        """x: windows [B_, N, C] -> [B_, N, C]; mask [nW, N, N] (0 / -100) or None."""
        b_, n, c = x.shape
        qkv = F.linear(x, self.qkv.weight, torch.cat((self.q_bias, self.k_bias.to(self.q_bias.dtype), self.v_bias)))
        q, k, v = qkv.reshape(b_, n, 3, self.num_heads, -1).permute(2, 0, 3, 1, 4).unbind(0)
        attn = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)
        attn = attn * self.logit_scales()
        bias = self.bias_table()[:, self.relative_position_index.view(-1)].view(self.num_heads, n, n)
        attn = attn + bias.unsqueeze(0)
        if mask is not None:
            nw = mask.shape[0]
            attn = (attn.view(-1, nw, self.num_heads, n, n) + mask.to(attn.dtype).unsqueeze(1).unsqueeze(0)).view(-1, self.num_heads, n, n)
        x = (attn.softmax(dim=-1) @ v).transpose(1, 2).reshape(b_, n, c)
        return self.proj(x)


class _SwinMlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class _SwinBlock(nn.Module):
    """timm 0.9.7 SwinTransformerV2Block (res-post-norm); the window is clamped to the map and the shift dropped when the window
    covers the map (_calc_window_shift)."""

    def __init__(self, dim, side, heads, window, shift, pretrained_window):
        super().__init__()
        self.side = side
        self.window = min(window, side)
        self.shift = 0 if side <= self.window else shift
        self.attn = _SwinAttention(dim, heads, self.window, pretrained_window)
        self.norm1 = nn.LayerNorm(dim)
        self.mlp = _SwinMlp(dim, 4 * dim)
        self.norm2 = nn.LayerNorm(dim)
        mask = None
        if self.shift:
            ws, s = self.window, self.shift
            img = torch.zeros((1, side, side, 1))
            cnt = 0
            for h in (slice(0, -ws), slice(-ws, -s), slice(-s, None)):
                for w in (slice(0, -ws), slice(-ws, -s), slice(-s, None)):
                    img[:, h, w, :] = cnt
                    cnt += 1
            mw = _window_partition(img, ws).view(-1, ws * ws)
            mask = mw.unsqueeze(1) - mw.unsqueeze(2)
            mask = mask.masked_fill(mask != 0, -100.0).masked_fill(mask == 0, 0.0)
        self.register_buffer("attn_mask", mask, persistent=False)

    def _load_from_state_dict(self, state_dict, prefix, *a, **k):
        state_dict.pop(prefix + "attn_mask", None)
        return super()._load_from_state_dict(state_dict, prefix, *a, **k)

    def _attn(self, x):
        b, h, w, c = x.shape
        ws, s = self.window, self.shift
        if s:
            x = torch.roll(x, shifts=(-s, -s), dims=(1, 2))
        win = self.attn(_window_partition(x, ws).view(-1, ws * ws, c), mask=self.attn_mask)
        x = _window_reverse(win.view(-1, ws, ws, c), ws, h, w)
        if s:
            x = torch.roll(x, shifts=(s, s), dims=(1, 2))
        return x

    def forward(self, x):
        x = x + self.norm1(self._attn(x))
        return x + self.norm2(self.mlp(x))


def _window_partition(x, ws):
    b, h, w, c = x.shape
    return x.view(b, h // ws, ws, w // ws, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws, ws, c)


def _window_reverse(win, ws, h, w):
    c = win.shape[-1]
    return win.view(-1, h // ws, w // ws, ws, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, h, w, c)


class _SwinPatchMerging(nn.Module):
    """timm 0.9.7 PatchMerging: 2 x 2 quads concatenated as (0, 0), (1, 0), (0, 1), (1, 1) (row, column), reduction, norm."""

    def __init__(self, dim):
        super().__init__()
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(2 * dim)

    def forward(self, x):
        b, h, w, c = x.shape
        x = x.reshape(b, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 4, 2, 5).flatten(3)
        return self.norm(self.reduction(x))


class _SwinStage(nn.Module):
    def __init__(self, dim, out_dim, side, depth, heads, window, pretrained_window, downsample):
        super().__init__()
        self.downsample = _SwinPatchMerging(dim) if downsample else nn.Identity()
        side = side // 2 if downsample else side
        self.side = side
        self.blocks = nn.ModuleList([_SwinBlock(out_dim, side, heads, window, 0 if i % 2 == 0 else window // 2, pretrained_window)
                                     for i in range(depth)])

    def forward(self, x):
        x = self.downsample(x)
        for blk in self.blocks:
            x = blk(x)
        return x


class _SwinPatchEmbed(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=SWIN_PATCH, stride=SWIN_PATCH)
        self.norm = nn.LayerNorm(dim)

    def forward(self, x):
        return self.norm(self.proj(x).permute(0, 2, 3, 1))


class _SwinV2Backbone(nn.Module):
    """timm SwinTransformerV2 with num_classes=0: forward(x [B, 3, 384, 384]) -> mean over tokens of norm(layers(patch_embed(x)))."""

    def __init__(self):
        super().__init__()
        self.img_size = SWIN_IMG
        self.num_features = SWIN_DIMS[-1]
        self.patch_embed = _SwinPatchEmbed(SWIN_DIMS[0])
        side = SWIN_IMG // SWIN_PATCH
        layers = []
        for i, (depth, dim, heads) in enumerate(zip(SWIN_DEPTHS, SWIN_DIMS, SWIN_HEADS)):
            layers.append(_SwinStage(SWIN_DIMS[max(i - 1, 0)], dim, side, depth, heads, SWIN_WINDOW, SWIN_PRETRAINED_WINDOWS[i],
                                     downsample=i > 0))
            side = layers[-1].side
        self.layers = nn.ModuleList(layers)
        self.norm = nn.LayerNorm(self.num_features)
        for m in self.modules():                                 # timm's initialisation
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward(self, x):
        if tuple(x.shape[-2:]) != (self.img_size, self.img_size):
            raise ValueError(f"SwinV2: input size ({x.shape[-2]}*{x.shape[-1]}) doesn't match model ({self.img_size}*{self.img_size})")
        x = self.patch_embed(x)
        for layer in self.layers:
            x = layer(x)
        return self.norm(x).mean(dim=(1, 2))


class _LinearView:
    """A Linear's weight with another bias (the qkv Linear with cat(q_bias, 0, v_bias)), duck-typed for _linear_terms."""

    def __init__(self, weight, bias):
        self.weight, self.bias = weight.detach(), bias
        self.out_features, self.in_features = weight.shape


class SwinV2(_Configurable, _InferenceCache, nn.Module):
    """Reference model.py:418-446 (SwinV2: `swinv2`, `fc`, unit-norm output), MI355X-native inference path."""

    def __init__(self, pretrained=False, embedding_dim=None, weights=None):
        super().__init__()
        if pretrained and weights is None:
            raise RuntimeError("pretrained=True needs a download in the reference (model.py:424-428); "
                               "pass weights=<state dict or path> instead")
        self.swinv2 = _SwinV2Backbone()
        self.fc = nn.Linear(self.swinv2.num_features, embedding_dim) if embedding_dim else None
        self._infer_cache = None
        self._init_config()
        if weights is not None:
            sd = torch.load(weights, map_location="cpu") if isinstance(weights, str) else weights
            for key in ("state-dict", "state_dict"):
                if isinstance(sd, dict) and key in sd:
                    sd = sd[key]
            self.load_state_dict(sd, strict=False)

    # -- the plain module graph (training, CPU tensors): same ops as timm ---------------------------------------------------
    def forward_eager(self, x):
        return torch.flatten(self.swinv2(x), 1)

    # -- MI355X inference path -------------------------------------------------------------------------------------------------
    def _watch_root(self):
        return self.swinv2

    def _prepare_inference(self):
        """Per block: the qkv view with its concatenated bias, the compact bias table, exp(clamp(logit_scale)) and the host-side
        bounds of every Linear's input (the residual stream's bound R: a stage starts at its LayerNorm's bound and every block adds
        the bounds of norm1 and norm2)."""
        bb = self.swinv2
        with torch.no_grad():
            r = _layernorm_bound(bb.patch_embed.norm)
            cache = {"r0": r, "stages": []}
            for stage in bb.layers:
                st = {"r_in": r, "blocks": []}
                if isinstance(stage.downsample, _SwinPatchMerging):
                    r = _layernorm_bound(stage.downsample.norm)
                for blk in stage.blocks:
                    at = blk.attn
                    c = at.dim
                    qkv = _LinearView(at.qkv.weight, torch.cat((at.q_bias, at.k_bias, at.v_bias)).detach().float().contiguous())
                    wv = at.qkv.weight.detach()[2 * c:].double()
                    # |attention output| <= max |v_j| <= ||x||_2 ||W_v,j||_2 + |b_j|, ||x||_2 <= sqrt(C) R
                    ba = math.sqrt(c) * r * float(torch.linalg.vector_norm(wv, dim=1).max()) + float(at.v_bias.detach().abs().max())
                    r1 = r + _layernorm_bound(blk.norm1)
                    w1 = blk.mlp.fc1
                    bh = (math.sqrt(c) * r1 * float(torch.linalg.vector_norm(w1.weight.detach().double(), dim=1).max())
                          + float(w1.bias.detach().abs().max()))                    # |gelu(v)| <= |v|
                    r2 = r1 + _layernorm_bound(blk.norm2)
                    st["blocks"].append({"qkv": qkv, "table": at.bias_table().detach().float().contiguous(),
                                         "ls": at.logit_scales().detach().float().reshape(-1).contiguous(),
                                         "r_qkv": r, "b_att": ba, "r_fc1": r1, "b_hid": bh, "r_out": r2})
                    r = r2
                cache["stages"].append(st)
        cache["_cuda"] = bb.patch_embed.proj.weight.is_cuda
        self._infer_cache = cache
        self._mark_built(cache)
        return cache

    def _features_native(self, x, cache):
        """x [b, 3, 384, 384] fp32 CUDA -> fp32 rows [b * 144, 1024] of the final LayerNorm (channels last)."""
        bb = self.swinv2
        lib = _lib.load()
        dev = x.device
        st_ = _stream(dev)
        b = x.shape[0]
        side = SWIN_IMG // SWIN_PATCH
        y = _conv_patch_tokens(bb.patch_embed.proj, x)                     # [b * 96 * 96, 128]
        xs = _terms_scale(cache["r0"])
        cur, xt = self._postnorm(None, y, bb.patch_embed.norm, xs)
        for si, (stage, sc) in enumerate(zip(bb.layers, cache["stages"])):
            if isinstance(stage.downsample, _SwinPatchMerging):
                ds = stage.downsample
                c = cur.shape[1]
                ms = _terms_scale(sc["r_in"])
                mt = torch.empty((b * (side // 2) ** 2, 4 * c * 2), dtype=torch.float16, device=dev)
                _lib.check(lib.mirx_patch_merge_terms(_ptr(cur), b, side, side, c, ms, _ptr(mt), st_), "mirx_patch_merge_terms")
                side //= 2
                y = _linear_terms(ds.reduction, mt, ms, (mt.shape[0],))
                del mt
                cur, xt = self._postnorm(None, y, ds.norm, _terms_scale(sc["blocks"][0]["r_qkv"]))
            for j, (blk, e) in enumerate(zip(stage.blocks, sc["blocks"])):
                at = blk.attn
                m, c = cur.shape
                last = j == len(stage.blocks) - 1
                xs = _terms_scale(e["r_qkv"])
                qkv = _linear_terms(e["qkv"], xt, xs, (m,))
                sa = _terms_scale(e["b_att"])
                att = torch.empty((m, 2 * c), dtype=torch.float16, device=dev)
                _lib.check(lib.mirx_window_attention_split2h(_ptr(qkv), b, side, blk.window, blk.shift, at.num_heads, c // at.num_heads,
                                                              _ptr(e["table"]), _ptr(e["ls"]), None, _ptr(att), sa, st_),
                           "mirx_window_attention_split2h")
                del qkv
                y = _linear_terms(at.proj, att, sa, (m,))
                del att
                s1 = _terms_scale(e["r_fc1"])
                cur, xt = self._postnorm(cur, y, blk.norm1, s1)
                ht, hs = _linear_terms(blk.mlp.fc1, xt, s1, (m,), act=1, terms_bound=e["b_hid"])
                y = _linear_terms(blk.mlp.fc2, ht, hs, (m,))
                del ht
                nxt = None if last else _terms_scale(sc["blocks"][j + 1]["r_qkv"])
                cur, xt = self._postnorm(cur, y, blk.norm2, nxt)
        return _layernorm(bb.norm, cur), side * side

    @staticmethod
    def _postnorm(x, y, ln, terms_scale):
        """[HIP] x + LayerNorm(y) (x None: LayerNorm(y)), in place into x; with terms_scale also as terms rows -> (out, terms)."""
        m, c = y.shape
        out = x if x is not None else torch.empty_like(y)
        t = torch.empty((m, 2 * c), dtype=torch.float16, device=y.device) if terms_scale is not None else None
        _lib.check(_lib.load().mirx_swin_postnorm(_ptr(x) if x is not None else None, _ptr(y), m, c, _ptr(ln.weight.detach()),
                                                  _ptr(ln.bias.detach()), float(ln.eps), _ptr(out), _ptr(t) if t is not None else None,
                                                  terms_scale if terms_scale is not None else 1.0, _stream(y.device)),
                   "mirx_swin_postnorm")
        return out, t

    def _embed_native(self, x, normalize, cache):
        b = x.shape[0]
        if b > SWIN_CHUNK:
            return torch.cat([self._embed_native(x[i:i + SWIN_CHUNK], normalize, cache) for i in range(0, b, SWIN_CHUNK)])
        rows, hw = self._features_native(x.contiguous(), cache)
        out = torch.empty((b, rows.shape[1]), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().mirx_gap_nhwc_l2norm(_ptr(rows), b, hw, rows.shape[1], 1 if normalize else 0, _ptr(out),
                                                    _stream(x.device)), "mirx_gap_nhwc_l2norm")
        return out

    def forward(self, x):
        if tuple(x.shape[-2:]) != (SWIN_IMG, SWIN_IMG) or x.dim() != 4:
            raise ValueError(f"SwinV2: input size ({x.shape[-2]}*{x.shape[-1]}) doesn't match model ({SWIN_IMG}*{SWIN_IMG}); "
                             f"the reference's transform gives {SWIN_IMG} x {SWIN_IMG}")
        native = x.is_cuda and not self.training and not torch.is_grad_enabled() and x.dtype == torch.float32
        if native:
            with torch.cuda.device(x.device):
                cache = self._cache()
                x = self._embed_native(x, self.fc is None, cache)
                if self.fc is None:
                    return x                       # already unit-norm (reference model.py:444)
                return _normalize_rows(_linear_auto(self.fc, x))        # [HIP] no library GEMM in a forward
        x = self.forward_eager(x)
        if self.fc:
            x = self.fc(x)
        return F.normalize(x, dim=1)


def build_model(model_type, embedding_dim=None, **kw):
    """Factory in the spirit of milvus_retrieval.py:143-162 (unknown type -> ValueError)."""
    if model_type == "densenet121":
        return DenseNet121(embedding_dim=embedding_dim, **kw), 224
    if model_type == "convnextv2":
        return ConvNeXtV2(embedding_dim=embedding_dim, **kw), 384
    if model_type == "dinov2":
        return DinoV2(embedding_dim=embedding_dim, **kw), 518
    if model_type == "medsiglip":
        return MedSigLIP(embed_dim=embedding_dim if embedding_dim is not None else 512, **kw), 448
    if model_type == "resnet50":
        return ResNet50(embedding_dim=embedding_dim, **kw), 224
    if model_type == "swinv2":
        return SwinV2(embedding_dim=embedding_dim, **kw), SWIN_IMG
    if model_type == "convnextv2_sra":
        # named in the reference's MODEL_CONFIGS (collection names), but its factory (milvus_retrieval.py:143-162) has no such
        # branch either: the reference builds the class directly (test.py:1172, ingest_embeddings.py:46), and so does a user here
        raise ValueError(f"Unknown model type: {model_type} (construct mirx.model.ConvNeXtV2_SRA(num_heads=.., lam=..) directly, "
                         f"as the reference does)")
    raise ValueError(f"Unknown model type: {model_type}")
