"""Tensor-level wrappers over the C ABI (include/mvs_hip.h).  Each function allocates its outputs with torch
(so the caching allocator owns them), enqueues the HIP kernels on the caller's current stream and returns
fresh tensors.  No autograd in here: the forward AND backward kernels of the training path are wrapped as plain functions
(*_bwd, *_wgrad, train_block_*, the losses); training.py builds the torch.autograd.Functions on top of them.

The bound library raises MvsHipError itself when a function the header declares mvs_status returns an error (_lib._GuardedLib),
so no call site checks a code.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib, packing
from ._lib import lib, ptr, stream_of


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


def _workspace(nbytes: int, device, unbuilt: Optional[str] = None) -> torch.Tensor:
    """The scratch buffer of a mvs_*_workspace_bytes query: uint8 (ptr() wants contiguity, no element type; the allocator aligns far
    beyond 8 bytes), rounded up past the next multiple of 16 so that it is never empty.  The C side is still told `nbytes`.  With
    `unbuilt` (the call's name) a query of zero means that nothing is built for the arguments, and raises."""
    if unbuilt is not None and not nbytes:
        raise _lib.MvsHipError("%s: not built for these arguments (or out of range)" % unbuilt)
    return torch.empty((nbytes // 16 + 1) * 16, dtype=torch.uint8, device=device)


class PackedFeatures:
    """Feature maps of one stage in the hand-off layout: ``data`` [B,V,C/8,H,W,8], fp32 / bf16 / fp16.
    Quacks like the [B,V,C,H,W] tensor the reference passes (``shape``, ``device``, ``dtype``) so StageNet.forward accepts either."""

    def __init__(self, data: torch.Tensor):
        assert data.dim() == 6 and data.shape[-1] == 8 and data.is_contiguous(), "PackedFeatures wants a dense [B,V,C/8,H,W,8] tensor"
        self.data = data

    @property
    def shape(self):
        B, V, O, H, W, _ = self.data.shape
        return torch.Size((B, V, O * 8, H, W))

    @property
    def device(self):
        return self.data.device

    @property
    def dtype(self):
        return self.data.dtype

    @property
    def requires_grad(self):
        return False

    def element_size(self):
        return self.data.element_size()

    def to(self, *a, **k):
        return PackedFeatures(self.data.to(*a, **k).contiguous())

    def unpack(self) -> torch.Tensor:
        """Back to planar [B,V,C,H,W] (tests / debugging)."""
        B, V, O, H, W, _ = self.data.shape
        return self.data.permute(0, 1, 2, 5, 3, 4).reshape(B, V, O * 8, H, W).contiguous()


def pack_features(features: torch.Tensor, dtype: Optional[torch.dtype] = None) -> PackedFeatures:
    """[B,V,C,H,W] (fp32 / bf16 / fp16) -> PackedFeatures in `dtype` (default: keep).  One read + one write of the features;
    a producer that emits the tiled layout itself has nothing to pack."""
    f, code = _feat(features)
    B, V, Cc, H, W = f.shape
    dtype = f.dtype if dtype is None else dtype
    out = torch.empty(B, V, Cc // 8, H, W, 8, dtype=dtype, device=f.device)
    lib().mvs_pack_features(ptr(f), code, ptr(out), _lib.DTYPE_CODE[dtype], B * V, Cc, H, W, stream_of(f))
    return PackedFeatures(out)


def feature_conv_is_built(cin: int, cout: int) -> bool:
    return bool(lib().mvs_feature_conv_is_built(int(cin), int(cout)))


def conv2d3x3_tiles(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], cout: int, swish: bool = False,
                    out: Optional[torch.Tensor] = None, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Producer-side feature emitter: x [N,Cin,H,W] planar (fp32 / bf16 / fp16; any batch stride) through
    Conv2d(Cin, cout, 3, padding=1) [+ bias] [+ Swish] -> octet tiles [N, cout/8, H, W, 8] in `dtype`, written by the convolution's
    epilogue (no planar output, no pack pass).  `out`: a [N, cout/8, H, W, 8] tensor or VIEW to fill - e.g. `packed.data[:, v]` of a
    [B, V, cout/8, H, W, 8] PackedFeatures buffer (any batch stride, the rest contiguous)."""
    if x.dtype not in _lib.DTYPE_CODE:
        x = x.float()
    N, cin, H, W = x.shape
    if x.stride()[1:] != (H * W, W, 1):
        x = x.contiguous()
    if out is None:
        out = torch.empty(N, cout // 8, H, W, 8, dtype=dtype, device=x.device)
    assert out.shape == (N, cout // 8, H, W, 8) and out.stride()[1:] == (H * W * 8, W * 8, 8, 1) and out.dtype in _lib.DTYPE_CODE, "tiled output [N,C/8,H,W,8]"
    lib().mvs_conv2d3x3_tiles_fwd(ptr(x), _lib.DTYPE_CODE[x.dtype], ptr(w_packed), ptr(bias), 1 if swish else 0, ptr(out), _lib.DTYPE_CODE[out.dtype],
                                  N, cin, cout, H, W, x.stride(0) if N > 1 else cin * H * W, out.stride(0) if N > 1 else cout * H * W, stream_of(x))
    return out


FPN_ACT_NONE, FPN_ACT_SWISH, FPN_ACT_LEAKY = 0, 1, 2


def fpn_conv_is_built(cin: int, cout: int, k: int, stride: int) -> bool:
    return bool(lib().mvs_fpn_conv_is_built(int(cin), int(cout), int(k), int(stride)))


def fpn_merge_is_built(clat: int, cout: int = 0) -> bool:
    return bool(lib().mvs_fpn_merge_is_built(int(clat), int(cout)))


def _planar32(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


def fpn_conv(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], cout: int, k: int, stride: int = 1,
             act: int = FPN_ACT_NONE) -> torch.Tensor:
    """FPN layer: x [N,Cin,H,W] -> act(Conv2d(Cin, cout, k, stride, padding k//2)(x) + bias) fp32
    [N, cout, (H-1)//stride+1, (W-1)//stride+1].  w_packed = packing.pack_fpn_conv_weights(w, stride) (BN folded); act = FPN_ACT_*."""
    x = _planar32(x)
    N, cin, H, W = x.shape
    out = torch.empty(N, cout, (H - 1) // stride + 1, (W - 1) // stride + 1, dtype=torch.float32, device=x.device)
    lib().mvs_fpn_conv_fwd(ptr(x), ptr(w_packed), ptr(bias), int(act), ptr(out), N, cin, int(cout), int(k), int(stride), H, W, stream_of(x))
    return out


def fpn_merge(prev: torch.Tensor, lateral: torch.Tensor, w_inner: torch.Tensor, b_inner: torch.Tensor) -> torch.Tensor:
    """FPNDecoder lateral merge (module.py:262-266): up2(prev [N,64,h,w]) + inner(lateral [N,Clat,2h,2w]) -> fp32 [N,64,2h,2w];
    inner = Conv2d(Clat, 64, 1) given as w_inner [64, Clat] fp32, b_inner [64]; up2 = bilinear x2, align_corners=True."""
    prev, lateral = _planar32(prev), _planar32(lateral)
    N, clat, H, W = lateral.shape
    assert prev.shape == (N, 64, H // 2, W // 2) and H % 2 == 0 and W % 2 == 0, (tuple(prev.shape), tuple(lateral.shape))
    out = torch.empty(N, 64, H, W, dtype=torch.float32, device=lateral.device)
    lib().mvs_fpn_merge_fwd(ptr(prev), ptr(lateral), ptr(_planar32(w_inner)), ptr(_planar32(b_inner)), ptr(out), N, clat, H, W, stream_of(lateral))
    return out


def fpn_merge_conv(prev: torch.Tensor, lateral: torch.Tensor, w_inner: torch.Tensor, b_inner: torch.Tensor, w_packed: torch.Tensor,
                   bias: Optional[torch.Tensor], cout: int, act: int = FPN_ACT_SWISH) -> torch.Tensor:
    """The decoder's last level fused (module.py:267-268): act(Conv2d(64, cout, 3, padding=1)(fpn_merge(prev, lateral, ...)) + bias)
    with the merged 64-channel map computed inside the convolution's staging (never written)."""
    prev, lateral = _planar32(prev), _planar32(lateral)
    N, clat, H, W = lateral.shape
    assert prev.shape == (N, 64, H // 2, W // 2) and H % 2 == 0 and W % 2 == 0, (tuple(prev.shape), tuple(lateral.shape))
    out = torch.empty(N, cout, H, W, dtype=torch.float32, device=lateral.device)
    lib().mvs_fpn_merge_conv_fwd(ptr(prev), ptr(lateral), ptr(_planar32(w_inner)), ptr(_planar32(b_inner)), ptr(w_packed), ptr(bias),
                                 int(act), ptr(out), N, clat, int(cout), H, W, stream_of(lateral))
    return out


# ---- FPNDecoder in train mode ----


def _planar_bn_fwd(entry, z, gamma, beta, eps, conv_bias, running_mean, running_var, momentum):
    """The body of the planar batch-statistics BatchNorm forwards; `entry` names the library's function (it fixes the activation)."""
    z = _planar32(z)
    N, C, H, W = z.shape
    L = lib()
    nbytes = L.mvs_fpn_bn_workspace_bytes(N, C, H, W)
    ws = _workspace(nbytes, z.device, unbuilt=entry)
    stats, y = torch.empty(3, C, dtype=torch.float32, device=z.device), torch.empty_like(z)
    getattr(L, entry)(ptr(z), ptr(conv_bias), ptr(gamma), ptr(beta), float(eps), float(momentum), ptr(running_mean), ptr(running_var),
                      ptr(stats), ptr(y), ptr(ws), nbytes, N, C, H, W, stream_of(z))
    return y, stats


def _planar_bn_bwd(entry, d_y, z, stats, gamma, beta):
    """The body of the planar BatchNorm backwards -> (d_z, d_gamma, d_beta)."""
    z, d_y = _planar32(z), _planar32(d_y)
    if d_y.shape != z.shape:
        raise ValueError("d_y must have z's shape %s; got %s" % (tuple(z.shape), tuple(d_y.shape)))
    N, C, H, W = z.shape
    L = lib()
    nbytes = L.mvs_fpn_bn_workspace_bytes(N, C, H, W)
    ws = _workspace(nbytes, z.device, unbuilt=entry)
    d_z = torch.empty_like(z)
    d_gamma, d_beta = torch.empty(C, dtype=torch.float32, device=z.device), torch.empty(C, dtype=torch.float32, device=z.device)
    getattr(L, entry)(ptr(d_y), ptr(z), ptr(stats), ptr(gamma), ptr(beta), ptr(d_z), ptr(d_gamma), ptr(d_beta), ptr(ws), nbytes,
                      N, C, H, W, stream_of(z))
    return d_z, d_gamma, d_beta


def _planar_wgrad(entry, what, variant, d_y, x, k, cols):
    """The body of the planar weight gradients: d_w [Cout, cols, k, k] on `entry`, built per (Cout, Cin, k, variant = `what`: ones | stride)."""
    N, cin, H, W = x.shape
    cout = d_y.shape[1]
    L = lib()
    nbytes = getattr(L, entry + "_workspace_bytes")(N, cin, cout, int(k), variant, H, W)
    ws = _workspace(nbytes, x.device, unbuilt="%s (Cout %d, Cin %d, k %d, %s %d)" % (entry, cout, cin, k, what, variant))
    d_w = torch.empty(cout, cols, k, k, dtype=torch.float32, device=x.device)
    getattr(L, entry)(ptr(d_y), ptr(x), ptr(d_w), ptr(ws), nbytes, N, cin, cout, int(k), variant, H, W, stream_of(x))
    return d_w


def fpn_bn_swish_fwd(z: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, conv_bias: Optional[torch.Tensor] = None,
                     running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None,
                     momentum: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Batch-statistics BatchNorm2d + Swish of a planar fp32 map z [N,C,H,W] (C <= 64) -> (y, stats [3, C] = mean | biased variance |
    invstd).  Given running_mean / running_var (fp32, contiguous; updated in place), one step of `momentum` with mean + conv_bias and the
    unbiased variance - what nn.BatchNorm2d does behind a convolution with that bias.  Sums in fp64, fixed order."""
    return _planar_bn_fwd("mvs_fpn_bn_swish_fwd", z, gamma, beta, eps, conv_bias, running_mean, running_var, momentum)


def fpn_bn_swish_bwd(d_y: torch.Tensor, z: torch.Tensor, stats: torch.Tensor, gamma: torch.Tensor,
                     beta: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Backward of fpn_bn_swish_fwd -> (d_z, d_gamma, d_beta)."""
    return _planar_bn_bwd("mvs_fpn_bn_swish_bwd", d_y, z, stats, gamma, beta)


def fpn_train_conv_is_built(cin: int, cout: int, k: int) -> bool:
    return bool(lib().mvs_fpn_train_conv_is_built(int(cin), int(cout), int(k)))


def fpn_train_conv(x: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Conv2d(Cin, Cout, k, padding k//2) of a planar map without bias or activation, w [Cout, Cin, k, k] fp32 (packed here, on its
    device): the FPNDecoder's data gradients (fpn_train_conv_is_built)."""
    x = _planar32(x)
    N, cin, H, W = x.shape
    cout, k = w.shape[0], w.shape[2]
    assert w.shape[1] == cin and w.shape[3] == k, (tuple(w.shape), cin)
    if out is None:
        out = torch.empty(N, cout, H, W, dtype=torch.float32, device=x.device)
    assert out.shape == (N, cout, H, W) and out.dtype == torch.float32
    wp = packing.pack_fpn_conv_weights(w, 1)
    lib().mvs_fpn_train_conv_fwd(ptr(x), ptr(wp), ptr(out), N, cin, cout, k, H, W, stream_of(x))
    return out


def fpn_wgrad(d_y: torch.Tensor, x: torch.Tensor, k: int, ones: bool = False) -> torch.Tensor:
    """d_w [Cout, Cin (+ 1), k, k] = the correlation of d_y [N,Cout,H,W] with x [N,Cin,H,W] (zero padding k//2), exact fp32 products;
    ones appends an input channel that is 1 inside the image (d_w[:, Cin] = the gradient of a bias behind the taps).  Deterministic."""
    d_y, x = _planar32(d_y), _planar32(x)
    N, cout, H, W = d_y.shape
    cin = x.shape[1]
    assert x.shape == (N, cin, H, W), (tuple(d_y.shape), tuple(x.shape))
    return _planar_wgrad("mvs_fpn_wgrad", "ones", int(ones), d_y, x, k, cin + int(ones))


def fpn_merge_wgrad(d_y: torch.Tensor, prev: torch.Tensor, lateral: torch.Tensor, w_inner: torch.Tensor, b_inner: torch.Tensor) -> torch.Tensor:
    """Weight gradient [8, 64, 3, 3] of the decoder's last 3x3 convolution: the correlation of d_y [N,8,H,W] with fpn_merge(prev, lateral,
    ...), which is re-evaluated inside the kernel and never written."""
    d_y, prev, lateral = _planar32(d_y), _planar32(prev), _planar32(lateral)
    N, clat, H, W = lateral.shape
    assert clat == 8 and prev.shape == (N, 64, H // 2, W // 2) and d_y.shape == (N, 8, H, W), (tuple(prev.shape), tuple(lateral.shape), tuple(d_y.shape))
    L = lib()
    nbytes = L.mvs_fpn_merge_wgrad_workspace_bytes(N, H, W)
    ws = _workspace(nbytes, lateral.device, unbuilt="mvs_fpn_merge_wgrad")
    d_w = torch.empty(8, 64, 3, 3, dtype=torch.float32, device=lateral.device)
    L.mvs_fpn_merge_wgrad(ptr(d_y), ptr(prev), ptr(lateral), ptr(_planar32(w_inner)), ptr(_planar32(b_inner)), ptr(d_w), ptr(ws), nbytes,
                          N, H, W, stream_of(lateral))
    return d_w


def fpn_up2_adjoint(d_fine: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The adjoint of fpn_merge's upsample: d_fine [N,64,H,W] -> [N,64,H/2,W/2], a gather over the forward's own taps."""
    d_fine = _planar32(d_fine)
    N, C, H, W = d_fine.shape
    assert C == 64 and H % 2 == 0 and W % 2 == 0, tuple(d_fine.shape)
    if out is None:
        out = torch.empty(N, 64, H // 2, W // 2, dtype=torch.float32, device=d_fine.device)
    assert out.shape == (N, 64, H // 2, W // 2) and out.dtype == torch.float32
    lib().mvs_fpn_up2_adjoint(ptr(d_fine), ptr(out), N, H, W, stream_of(d_fine))
    return out


# ---- FPNEncoder in train mode ----


def fpn_bn_leaky_fwd(z: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, running_mean: Optional[torch.Tensor] = None,
                     running_var: Optional[torch.Tensor] = None, momentum: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Batch-statistics BatchNorm2d + leaky_relu(0.1) of a planar fp32 map z [N,C,H,W] (C <= 64) -> (y, stats [3, C] = mean | biased
    variance | invstd); running statistics as in fpn_bn_swish_fwd (the encoder's convolutions have no bias).  Sums in fp64, fixed order."""
    return _planar_bn_fwd("mvs_fpn_bn_leaky_fwd", z, gamma, beta, eps, None, running_mean, running_var, momentum)


def fpn_bn_leaky_bwd(d_y: torch.Tensor, z: torch.Tensor, stats: torch.Tensor, gamma: torch.Tensor,
                     beta: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Backward of fpn_bn_leaky_fwd -> (d_z, d_gamma, d_beta); du = dy (u > 0 ? 1 : 0.1) with u recomputed from z and stats."""
    return _planar_bn_bwd("mvs_fpn_bn_leaky_bwd", d_y, z, stats, gamma, beta)


def fpn_enc_wgrad(d_y: torch.Tensor, x: torch.Tensor, k: int, stride: int = 1) -> torch.Tensor:
    """d_w [Cout, Cin, k, k] of Conv2d(Cin, Cout, k, stride, padding k//2): the correlation of d_y [N,Cout,OH,OW] with x [N,Cin,H,W], exact
    fp32 products; built for the FPNEncoder's eight distinct layers.  Deterministic."""
    d_y, x = _planar32(d_y), _planar32(x)
    N, cin, H, W = x.shape
    cout = d_y.shape[1]
    if d_y.shape != (N, cout, (H - 1) // stride + 1, (W - 1) // stride + 1):
        raise ValueError("d_y %s does not belong to x %s at stride %d" % (tuple(d_y.shape), tuple(x.shape), stride))
    return _planar_wgrad("mvs_fpn_enc_wgrad", "stride", int(stride), d_y, x, k, cin)


def fpn_enc_dgrad_is_built(cin: int, cout: int, k: int, stride: int) -> bool:
    """Stride 1: the inference list's Cin = Cout instance; stride 2: the parity-class kernels."""
    if stride == 1:
        return cin == cout and fpn_conv_is_built(cin, cout, k, 1)
    return bool(lib().mvs_fpn_enc_dgrad_is_built(int(cin), int(cout), int(k), int(stride)))


def fpn_enc_dgrad(d_z: torch.Tensor, w: torch.Tensor, stride: int = 1) -> torch.Tensor:
    """d_x of Conv2d(Cin, Cout, k, stride, padding k//2) with weight w [Cout, Cin, k, k] (fp32; packed here, on its device) from d_z
    [N,Cout,OH,OW].  Stride 1 (Cin = Cout): mvs_fpn_conv_fwd on the flipped, channel-transposed taps -> [N,Cin,OH,OW].  Stride 2: the four
    parity classes of the transposed convolution (mvs_fpn_enc_dgrad) -> [N,Cin,2 OH,2 OW]."""
    d_z = _planar32(d_z)
    N, cout, OH, OW = d_z.shape
    cin, k = w.shape[1], w.shape[2]
    if w.shape[0] != cout or w.shape[3] != k:
        raise ValueError("w %s does not belong to d_z %s" % (tuple(w.shape), tuple(d_z.shape)))
    if not fpn_enc_dgrad_is_built(cin, cout, k, stride):
        raise _lib.MvsHipError("mvs_fpn_enc_dgrad: not built for (Cin %d, Cout %d, k %d, stride %d)" % (cin, cout, k, stride))
    if stride == 1:
        return fpn_conv(d_z, packing.pack_fpn_conv_weights(w.float().flip(2, 3).transpose(0, 1).contiguous(), 1), None, cin, k, 1, FPN_ACT_NONE)
    wp = packing.pack_fpn_enc_dgrad_weights(w)
    assert wp.numel() * wp.element_size() == lib().mvs_fpn_enc_dgrad_weights_bytes(cin, cout, k), (wp.numel(), cin, cout, k)
    d_x = torch.empty(N, cin, 2 * OH, 2 * OW, dtype=torch.float32, device=d_z.device)
    lib().mvs_fpn_enc_dgrad(ptr(d_z), ptr(wp), ptr(d_x), N, cin, cout, k, 2 * OH, 2 * OW, stream_of(d_z))
    return d_x


def _fmt_tokens(x: torch.Tensor) -> torch.Tensor:
    x = _planar32(x)
    if x.dim() < 3 or x.shape[1] != 64:
        raise ValueError("FMT tokens are planar [N, 64, n] (or the feature map [N, 64, h, w]); got %s" % (tuple(x.shape),))
    return x


def _fmt_params(w_packed: torch.Tensor, vectors: torch.Tensor) -> None:
    L = lib()
    if w_packed.numel() * w_packed.element_size() != L.mvs_fmt_weights_bytes() or vectors.dtype != torch.float32 \
            or vectors.numel() * 4 != L.mvs_fmt_vectors_bytes():
        raise ValueError("(w_packed, vectors) must come from packing.pack_fmt_block")


def _fmt_pe(pe: Optional[torch.Tensor], x: torch.Tensor) -> None:
    n = x[0, 0].numel()
    if pe is not None and (pe.dtype != torch.float32 or tuple(pe.shape) != (64, n) or not pe.is_contiguous() or pe.device != x.device):
        raise ValueError("pe must be the fp32 contiguous position table [64, %d] of this map size on %s; got %s %s on %s"
                         % (n, x.device, pe.dtype, tuple(pe.shape), pe.device))


def _fmt_smooth_weights(w_packed: torch.Tensor, C: int) -> None:
    """w_packed must be packing.pack_fpn_conv_weights(w [C, C, 3, 3], 1): [steps][row blocks][hi|lo][64 lanes][8] bf16."""
    want = ((9 * (C // 8) + 3) // 4) * ((C + 15) // 16) * 2 * 64 * 8 * 2
    if C % 8 == 0 and w_packed.numel() * w_packed.element_size() != want:
        raise ValueError("w_packed must come from packing.pack_fpn_conv_weights(w [%d, %d, 3, 3], 1): %d bytes, got %d"
                         % (C, C, want, w_packed.numel() * w_packed.element_size()))


def fmt_kv(x: torch.Tensor, w_packed: torch.Tensor, vectors: torch.Tensor, pe: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Key/value summary of one FMT block: x [N, 64, n] or [N, 64, h, w] planar (+ pe [64, n]) -> the packed
    operand [N, mvs_fmt_kv_operand_bytes] (uint8) that fmt_block consumes: KV_h = sum_s k_s (x) v_s and sum_s k_s of LN1(x), k = elu(Wk .) + 1.
    (w_packed, vectors) = packing.pack_fmt_block.  Deterministic (fixed-order reduction, no atomics)."""
    x = _fmt_tokens(x)
    _fmt_params(w_packed, vectors)
    _fmt_pe(pe, x)
    N, n = x.shape[0], x[0, 0].numel()
    L = lib()
    ws_bytes = L.mvs_fmt_kv_workspace_bytes(N, n)
    ws = _workspace(ws_bytes, x.device)
    out = torch.empty(N, L.mvs_fmt_kv_operand_bytes(), dtype=torch.uint8, device=x.device)
    L.mvs_fmt_kv_fwd(ptr(x), ptr(pe), ptr(w_packed), ptr(vectors), ptr(ws), ws_bytes, ptr(out), N, n, stream_of(x))
    return out


def fmt_block(x: torch.Tensor, kv_operand: torch.Tensor, w_packed: torch.Tensor, vectors: torch.Tensor, pe: Optional[torch.Tensor] = None,
              kv_div: int = 1) -> torch.Tensor:
    """One pre-norm CrossBlock with linear attention for N views in one launch: x [N, 64, n] or [N, 64, h, w] (+ pe) -> the same shape,
    fp32.  View i attends to kv_operand[i // kv_div] (fmt_kv of x itself for self attention, of the reference view's tokens for cross
    attention with kv_div = V - 1)."""
    x = _fmt_tokens(x)
    _fmt_params(w_packed, vectors)
    _fmt_pe(pe, x)
    N, n = x.shape[0], x[0, 0].numel()
    assert kv_div >= 1 and kv_operand.shape[0] * kv_div >= N and kv_operand.shape[1] == lib().mvs_fmt_kv_operand_bytes(), \
        (tuple(kv_operand.shape), kv_div, N)
    out = torch.empty_like(x)
    lib().mvs_fmt_block_fwd(ptr(x), ptr(pe), ptr(kv_operand), ptr(w_packed), ptr(vectors), ptr(out), N, n, int(kv_div), stream_of(x))
    return out


def _fmt_level(prev: torch.Tensor, lateral: torch.Tensor, w_reduce: torch.Tensor):
    prev, lateral = _planar32(prev), _planar32(lateral)
    N, C, H, W = lateral.shape
    assert prev.dim() == 4 and prev.shape[:2] == (N, 2 * C) and tuple(w_reduce.shape) == (C, 2 * C), (tuple(prev.shape), tuple(lateral.shape))
    return prev, lateral, _planar32(w_reduce), N, C, prev.shape[2], prev.shape[3], H, W


def fmt_path(prev: torch.Tensor, lateral: torch.Tensor, w_reduce: torch.Tensor, w_packed: torch.Tensor) -> torch.Tensor:
    """One pathway level fused (FMT.py:195-197): smooth(bilinear(dim_reduction(prev [N,2C,h,w]), size (H,W), align_corners=False) + lateral
    [N,C,H,W]) -> [N,C,H,W] fp32; w_reduce [C,2C], w_packed = packing.pack_fpn_conv_weights(smooth.weight, 1).  The merged map is
    computed inside the convolution's staging and never written."""
    prev, lateral, w_reduce, N, C, h, w, H, W = _fmt_level(prev, lateral, w_reduce)
    _fmt_smooth_weights(w_packed, C)
    out = torch.empty_like(lateral)
    lib().mvs_fmt_path_fwd(ptr(prev), ptr(lateral), ptr(w_reduce), ptr(w_packed), ptr(out), N, C, h, w, H, W, stream_of(lateral))
    return out


def fmt_merge(prev: torch.Tensor, lateral: torch.Tensor, w_reduce: torch.Tensor) -> torch.Tensor:
    """The merged map of a pathway level, written out (the unfused form): bilinear(dim_reduction(prev)) + lateral -> [N,C,H,W] fp32."""
    prev, lateral, w_reduce, N, C, h, w, H, W = _fmt_level(prev, lateral, w_reduce)
    out = torch.empty_like(lateral)
    lib().mvs_fmt_merge_fwd(ptr(prev), ptr(lateral), ptr(w_reduce), ptr(out), N, C, h, w, H, W, stream_of(lateral))
    return out


def fmt_smooth(x: torch.Tensor, w_packed: torch.Tensor) -> torch.Tensor:
    """Conv2d(C, C, 3, padding=1, bias=False) of the pathway (smooth_k) on a planar map [N,C,H,W], C = 32 | 16 | 8 -> fp32."""
    x = _planar32(x)
    N, C, H, W = x.shape
    _fmt_smooth_weights(w_packed, C)
    out = torch.empty_like(x)
    lib().mvs_fmt_smooth_fwd(ptr(x), ptr(w_packed), ptr(out), N, C, H, W, stream_of(x))
    return out


def _fmt_level_grad(grad: torch.Tensor, lateral_shape, what: str) -> torch.Tensor:
    grad = _planar32(grad)
    if tuple(grad.shape) != tuple(lateral_shape):
        raise ValueError("%s must have the lateral's shape %s; got %s" % (what, tuple(lateral_shape), tuple(grad.shape)))
    return grad


def fmt_path_bwd(d_merged: torch.Tensor, prev: torch.Tensor, w_reduce: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Backward of a pathway level's merge: d_merged [N,C,H,W] (the gradient of bilinear(dim_reduction(prev)) +
    lateral, which is also the lateral's) -> (d_prev [N,2C,h,w], d_w_reduce [C,2C]) fp32.  The interpolation's adjoint is a gather over
    the forward's own taps; deterministic (fixed-order reduction, no atomics)."""
    prev, d_merged, w_reduce, N, C, h, w, H, W = _fmt_level(prev, d_merged, w_reduce)
    L = lib()
    ws_bytes = L.mvs_fmt_path_bwd_workspace_bytes(N, C, h, w)
    ws = _workspace(ws_bytes, prev.device)
    d_prev, d_w = torch.empty_like(prev), torch.empty(C, 2 * C, dtype=torch.float32, device=prev.device)
    L.mvs_fmt_path_bwd(ptr(d_merged), ptr(prev), ptr(w_reduce), ptr(d_prev), ptr(d_w), ptr(ws), ws_bytes, N, C, h, w, H, W, stream_of(prev))
    return d_prev, d_w


def fmt_smooth_wgrad(d_y: torch.Tensor, prev: torch.Tensor, lateral: torch.Tensor, w_reduce: torch.Tensor) -> torch.Tensor:
    """Weight gradient of a pathway level's smooth_k: d_y [N,C,H,W] -> d_w [C,C,3,3] fp32 = the correlation of
    d_y with the merged map, which is recomputed from (prev, lateral, w_reduce) inside the kernel and never written.  Exact fp32
    products; deterministic."""
    prev, lateral, w_reduce, N, C, h, w, H, W = _fmt_level(prev, lateral, w_reduce)
    d_y = _fmt_level_grad(d_y, lateral.shape, "d_y")
    L = lib()
    ws_bytes = L.mvs_fmt_smooth_wgrad_workspace_bytes(N, C, H, W)
    ws = _workspace(ws_bytes, lateral.device)
    d_w = torch.empty(C, C, 3, 3, dtype=torch.float32, device=lateral.device)
    L.mvs_fmt_smooth_wgrad(ptr(d_y), ptr(prev), ptr(lateral), ptr(w_reduce), ptr(d_w), ptr(ws), ws_bytes, N, C, h, w, H, W, stream_of(lateral))
    return d_w


VITDEC_EPI_F32, VITDEC_EPI_RESID, VITDEC_EPI_GELU_SPLIT = 0, 1, 2
VITDEC_PROJ, VITDEC_UP0, VITDEC_UP1 = 0, 1, 2
_VITDEC_CONV = {VITDEC_PROJ: (768, 256, 9, 1), VITDEC_UP0: (256, 128, 4, 4), VITDEC_UP1: (128, 64, 4, 4)}     # Cin, Cout, taps, classes


def _base_ptr(t: torch.Tensor):
    """Address of element 0 of a tensor that may be strided (the device checks of ptr() on a one-element view of it)."""
    return ptr(t.as_strided((1,), (1,)))


def _vitdec_packed(t: Optional[torch.Tensor], rows: int, channels: int, what: str) -> None:
    want = lib().mvs_vitdec_packed_bytes(rows, channels)
    if t is None or t.dtype != torch.uint8 or t.dim() != 1 or t.numel() != want or not t.is_contiguous():
        raise ValueError("%s must be a packed-split uint8 tensor of mvs_vitdec_packed_bytes(%d, %d) = %d bytes; got %s"
                         % (what, rows, channels, want, None if t is None else (t.dtype, tuple(t.shape))))


def _vitdec_vec(t: Optional[torch.Tensor], n: int, what: str, like: torch.Tensor) -> None:
    if t is None or t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous() or t.device != like.device:
        raise ValueError("%s must be a contiguous fp32 vector of %d elements on %s; got %s"
                         % (what, n, like.device, None if t is None else (t.dtype, tuple(t.shape), t.device)))


def vitdec_rows(inp: torch.Tensor, v0: int, views: int, *, prev: Optional[torch.Tensor] = None, prev_value: Optional[torch.Tensor] = None,
                mix: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ln: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                want_x: bool = True, packed_into: Optional[torch.Tensor] = None, want_packed: bool = False, out_V: Optional[int] = None,
                out_v0: int = 0):
    """Row pass of the ViT decoder.  inp [B, Vall, n, 768] (fp32 / bf16 / fp16; ANY batch / view / row stride,
    the 768 channels contiguous: it is read in place, nothing is copied): the rows of views v0 .. v0 + views - 1, M = B views n.
    value = [prev_value * prev [M, 768] +] inp [-> LayerNorm(mix, eps 1e-6)].  Returns (x fp32 [M, 768] or None, x packed-split or None,
    packed-split LayerNorm(ln, eps 1e-5)(x) or None).  The packed x goes to row (b * out_V + out_v0 + j) * n + t of `packed_into`
    (default: a fresh buffer with out_V = views)."""
    if inp.dim() != 4 or inp.shape[3] != 768 or inp.stride(3) != 1 or inp.dtype not in _lib.DTYPE_CODE or inp.stride(2) < 768 \
            or inp.stride(0) < 0 or inp.stride(1) < 0:
        raise ValueError("vitdec_rows takes [B, V, n, 768] fp32 / bf16 / fp16 with contiguous channels and rows that do not overlap (row stride >= 768); got %s %s strides %s"
                         % (inp.dtype, tuple(inp.shape), tuple(inp.stride())))
    B, Vall, n = inp.shape[:3]
    if not (0 <= v0 and views >= 1 and v0 + views <= Vall and n >= 1):
        raise ValueError("views %d .. %d of %d" % (v0, v0 + views - 1, Vall))
    M = B * views * n
    if prev is not None:
        if prev.dtype != torch.float32 or tuple(prev.shape) != (M, 768) or not prev.is_contiguous():
            raise ValueError("prev must be contiguous fp32 [%d, 768]; got %s %s" % (M, prev.dtype, tuple(prev.shape)))
        _vitdec_vec(prev_value, 1, "prev_value", inp)
    for pair, what in ((mix, "mix"), (ln, "ln")):
        if pair is not None:
            _vitdec_vec(pair[0], 768, what + " weight", inp)
            _vitdec_vec(pair[1], 768, what + " bias", inp)
    L = lib()
    out_V = views if out_V is None else int(out_V)
    xp = packed_into
    if want_packed or xp is not None:
        if out_v0 < 0 or out_V < out_v0 + views:
            raise ValueError("out_V %d cannot hold views %d .. %d" % (out_V, out_v0, out_v0 + views - 1))
        if xp is None:
            xp = torch.empty(L.mvs_vitdec_packed_bytes(B * out_V * n, 768), dtype=torch.uint8, device=inp.device)
        _vitdec_packed(xp, B * out_V * n, 768, "packed_into")
    if not (want_x or xp is not None or ln is not None):
        raise ValueError("vitdec_rows: nothing to compute")
    x = torch.empty(M, 768, dtype=torch.float32, device=inp.device) if want_x else None
    xn = torch.empty(L.mvs_vitdec_packed_bytes(M, 768), dtype=torch.uint8, device=inp.device) if ln is not None else None
    L.mvs_vitdec_rows_fwd(_base_ptr(inp), _lib.DTYPE_CODE[inp.dtype], inp.stride(0), inp.stride(1), inp.stride(2), int(v0), int(views), ptr(prev),
                          ptr(prev_value) if prev is not None else None, ptr(mix[0]) if mix else None, ptr(mix[1]) if mix else None, ptr(x), ptr(xp),
                          out_V, int(out_v0), ptr(ln[0]) if ln else None, ptr(ln[1]) if ln else None, ptr(xn), B * views, n, 768, stream_of(inp))
    return x, xp, xn


def vitdec_linear(a_packed: torch.Tensor, M: int, w_packed: torch.Tensor, K: int, N: int, epilogue: int, *, bias: Optional[torch.Tensor] = None,
                  gamma: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, elu_cols: int = 0) -> torch.Tensor:
    """y = epilogue(a W^T): a packed-split [M, K], w_packed = packing.pack_linear_bf16x3(W [N, K]).  VITDEC_EPI_F32 -> fp32 [M, N] with
    elu(.) + 1 on columns < elu_cols; VITDEC_EPI_RESID -> fp32 residual + gamma * (. + bias); VITDEC_EPI_GELU_SPLIT -> packed-split
    GELU(. + bias)."""
    _vitdec_packed(a_packed, M, K, "a_packed")
    if w_packed.dtype != torch.bfloat16 or w_packed.numel() != 2 * K * N or not w_packed.is_contiguous():
        raise ValueError("w_packed must come from packing.pack_linear_bf16x3(W [%d, %d]): %d bf16 elements, got %s %d"
                         % (N, K, 2 * K * N, w_packed.dtype, w_packed.numel()))
    if bias is not None:
        _vitdec_vec(bias, N, "bias", a_packed)
    if epilogue == VITDEC_EPI_RESID:
        _vitdec_vec(bias, N, "bias", a_packed)
        _vitdec_vec(gamma, N, "gamma", a_packed)
        if residual is None or residual.dtype != torch.float32 or tuple(residual.shape) != (M, N) or not residual.is_contiguous():
            raise ValueError("residual must be contiguous fp32 [%d, %d]" % (M, N))
    if epilogue == VITDEC_EPI_GELU_SPLIT:
        out = torch.empty(lib().mvs_vitdec_packed_bytes(M, N), dtype=torch.uint8, device=a_packed.device)
    else:
        out = torch.empty(M, N, dtype=torch.float32, device=a_packed.device)
    lib().mvs_vitdec_linear_fwd(ptr(a_packed), ptr(w_packed), ptr(bias), ptr(gamma), ptr(residual), ptr(out), int(M), int(K), int(N),
                                int(epilogue), int(elu_cols), stream_of(a_packed))
    return out


def vitdec_kv(kv: torch.Tensor, NV: int, n: int) -> torch.Tensor:
    """Key/value summary: kv fp32 [NV * n, 1536] (elu(k) + 1 | v) -> fp32 [NV, 12, 64 * 64 + 64] = per head KV_h [d][m] | ksum_h [d],
    from exact fp32 products, per-slab partials added in a fixed order (no atomics: bit-identical run to run)."""
    if kv.dtype != torch.float32 or kv.dim() != 2 or kv.shape[0] != NV * n or not kv.is_contiguous():
        raise ValueError("kv must be contiguous fp32 [NV * n, 1536]; got %s %s" % (kv.dtype, tuple(kv.shape)))
    L = lib()
    ws_bytes = L.mvs_vitdec_kv_workspace_bytes(NV, n)
    ws = _workspace(ws_bytes, kv.device)
    out = torch.empty(NV, 12, 64 * 64 + 64, dtype=torch.float32, device=kv.device)
    L.mvs_vitdec_kv_fwd(ptr(kv), ptr(ws), ws_bytes, ptr(out), NV, n, kv.shape[1], stream_of(kv))
    return out


def vitdec_apply(q: torch.Tensor, summary: torch.Tensor, NV: int, n: int, kv_div: int = 1) -> torch.Tensor:
    """a = (q . KV_h) / (q . ksum_h + 1e-6) per head: q fp32 [NV * n, 768] (elu + 1 applied); view i uses summary[i // kv_div] ->
    packed-split [NV * n, 768]."""
    if q.dtype != torch.float32 or q.dim() != 2 or q.shape[0] != NV * n or not q.is_contiguous():
        raise ValueError("q must be contiguous fp32 [NV * n, 768]; got %s %s" % (q.dtype, tuple(q.shape)))
    if summary.dtype != torch.float32 or summary.dim() != 3 or tuple(summary.shape[1:]) != (12, 4160) or not summary.is_contiguous() \
            or kv_div < 1 or summary.shape[0] * kv_div < NV:
        raise ValueError("summary must be vitdec_kv's fp32 [NVkv, 12, 4160] with NVkv * kv_div >= NV; got %s, kv_div %d, NV %d"
                         % (tuple(summary.shape), kv_div, NV))
    out = torch.empty(lib().mvs_vitdec_packed_bytes(NV * n, 768), dtype=torch.uint8, device=q.device)
    lib().mvs_vitdec_apply_fwd(ptr(q), ptr(summary), ptr(out), NV, n, int(kv_div), q.shape[1], stream_of(q))
    return out


def vitdec_conv(x_packed: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, layer: int, NV: int, H: int, W: int,
                planar: bool = False) -> torch.Tensor:
    """proj (VITDEC_PROJ: Conv2d 768 -> 256, 3x3) / upsampler0, upsampler1 (VITDEC_UP0 / UP1: ConvTranspose2d 4x4 stride 2 padding 1) with
    folded BatchNorm and SiLU on packed-split tokens of the [NV, H, W] map -> packed-split tokens of the output map, or planar fp32
    [NV, Cout, Ho, Wo].  (w_packed, bias) = packing.pack_vitdec_conv / pack_vitdec_deconv."""
    if layer in _VITDEC_CONV:
        cin, cout, taps, classes = _VITDEC_CONV[layer]
        _vitdec_packed(x_packed, NV * H * W, cin, "x_packed")
        want = classes * taps * cin * ((cout + 127) // 128 * 128) * 2
        if w_packed.dtype != torch.bfloat16 or w_packed.numel() != want or not w_packed.is_contiguous():
            raise ValueError("w_packed must come from packing.pack_vitdec_%s: %d bf16 elements, got %s %d"
                             % ("conv" if layer == VITDEC_PROJ else "deconv", want, w_packed.dtype, w_packed.numel()))
        _vitdec_vec(bias, cout, "bias", x_packed)
        s = 1 if layer == VITDEC_PROJ else 2
        if planar:
            out = torch.empty(NV, cout, s * H, s * W, dtype=torch.float32, device=x_packed.device)
        else:
            out = torch.empty(lib().mvs_vitdec_packed_bytes(NV * s * H * s * W, cout), dtype=torch.uint8, device=x_packed.device)
    else:
        out = torch.empty(1, dtype=torch.uint8, device=x_packed.device)       # the library refuses the layer
    lib().mvs_vitdec_conv_fwd(ptr(x_packed), ptr(w_packed), ptr(bias), ptr(out), int(layer), 1 if planar else 0, NV, H, W, stream_of(x_packed))
    return out


# ---- training of the CrossVITDecoder's blocks (csrc/vitdec_train_kernels.hip) ----
def _vitdec_tokens(t: torch.Tensor, cols: Optional[int], what: str) -> None:
    if t is None or t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or t.shape[0] < 1 or (cols is not None and t.shape[1] != cols):
        raise ValueError("%s must be contiguous fp32 [M, %s]; got %s" % (what, "C" if cols is None else cols,
                                                                          None if t is None else (t.dtype, tuple(t.shape))))


def vitdec_wgrad_slabs(M: int, N: int, K: int) -> int:
    """Token slabs of vitdec_wgrad's launch at these sizes; 0 = not built.  The header states the workspace as slabs * (N K + N) floats;
    the ABI's naming rule leaves no room for a count that is neither a status nor a size, so it is read off that size."""
    return lib().mvs_vitdec_wgrad_workspace_bytes(int(M), int(N), int(K)) // ((N * K + N) * 4)


def vitdec_wgrad(dy: torch.Tensor, x: torch.Tensor, want_bias: bool = False):
    """Weight gradient of a linear layer over tokens: dy fp32 [M, N], x fp32 [M, K] -> dw fp32 [N, K] = dy^T x (three-term split-bf16
    products, per-slab partials added in slab order: no atomics), and with want_bias (dw, dbias [N] = column sums of dy)."""
    _vitdec_tokens(dy, None, "dy")
    _vitdec_tokens(x, None, "x")
    if x.shape[0] != dy.shape[0] or x.device != dy.device:
        raise ValueError("dy %s and x %s must have the same rows and device" % (tuple(dy.shape), tuple(x.shape)))
    M, N, K = dy.shape[0], dy.shape[1], x.shape[1]
    L = lib()
    ws_bytes = L.mvs_vitdec_wgrad_workspace_bytes(M, N, K)
    ws = _workspace(ws_bytes, dy.device, unbuilt="mvs_vitdec_wgrad: built for N and K multiples of 128 (dw [%d, %d])" % (N, K))
    dw = torch.empty(N, K, dtype=torch.float32, device=dy.device)
    db = torch.empty(N, dtype=torch.float32, device=dy.device) if want_bias else None
    L.mvs_vitdec_wgrad(ptr(dy), ptr(x), ptr(dw), ptr(db), ptr(ws), ws_bytes, M, N, K, stream_of(dy))
    return (dw, db) if want_bias else dw


def vitdec_ln_bwd(d_y: torch.Tensor, x: torch.Tensor, w: torch.Tensor, eps: float, add: Optional[torch.Tensor] = None):
    """LayerNorm backward over rows of 768: d_y, x fp32 [M, 768], w [768] -> (d_x [+ add], d_w, d_b); mean and rstd are recomputed from
    x, d_w / d_b come from per-workgroup partials added in a fixed order."""
    _vitdec_tokens(d_y, 768, "d_y")
    _vitdec_tokens(x, 768, "x")
    if add is not None:
        _vitdec_tokens(add, 768, "add")
    M = d_y.shape[0]
    if x.shape[0] != M or (add is not None and add.shape[0] != M):
        raise ValueError("d_y, x and add must have the same rows")
    _vitdec_vec(w, 768, "w", d_y)
    L = lib()
    ws_bytes = L.mvs_vitdec_ln_bwd_workspace_bytes(M, 768)
    ws = _workspace(ws_bytes, d_y.device)
    d_x = torch.empty_like(d_y)
    d_wb = torch.empty(2, 768, dtype=torch.float32, device=d_y.device)
    L.mvs_vitdec_ln_bwd(ptr(d_y), ptr(x), ptr(w), float(eps), ptr(add), ptr(d_x), ptr(d_wb), ptr(ws), ws_bytes, M, 768, stream_of(d_y))
    return d_x, d_wb[0], d_wb[1]


def vitdec_pack(x: torch.Tensor) -> torch.Tensor:
    """fp32 [M, C] (C = 768 | 1536 | 3072) -> the packed-split row operand of vitdec_linear."""
    _vitdec_tokens(x, None, "x")
    M, C = x.shape
    if C not in (768, 1536, 3072):
        raise ValueError("vitdec_pack is built for rows of 768, 1536 or 3072 channels; got %d" % C)
    out = torch.empty(lib().mvs_vitdec_packed_bytes(M, C), dtype=torch.uint8, device=x.device)
    lib().mvs_vitdec_pack_fwd(ptr(x), ptr(out), M, C, stream_of(x))
    return out


def vitdec_dgrad(dy: torch.Tensor, wt_packed: torch.Tensor, N_in: int, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Data gradient of a linear layer y = x W^T (W [N_out, N_in]): dy fp32 [M, N_out] -> dx fp32 [M, N_in] = dy W, the forward GEMM on
    wt_packed = packing.pack_linear_bf16x3(W.t())."""
    return vitdec_linear(vitdec_pack(dy), dy.shape[0], wt_packed, dy.shape[1], N_in, VITDEC_EPI_F32, bias=bias)


# ---- training of the CrossVITDecoder's head (csrc/vitdec_head_train_kernels.hip) ----
# [NV, H, W] is always the layer's INPUT map; the output map of VITDEC_UP0 / UP1 has 4 NV H W rows in fine-map order.
def _vitdec_head_rows(layer: int, NV: int, H: int, W: int) -> Tuple[int, int]:
    """(rows of the layer's input map, rows of its output map)"""
    if layer not in _VITDEC_CONV:
        return 1, 1                                                    # the library refuses the layer
    M = NV * H * W
    return M, M if layer == VITDEC_PROJ else 4 * M


def vitdec_head_conv(x_packed: torch.Tensor, w_packed: torch.Tensor, layer: int, NV: int, H: int, W: int) -> torch.Tensor:
    """Pre-activation of a head layer in train mode: the convolution of the packed-split tokens of the [NV, H, W] map with the RAW weights
    and no bias -> fp32 [output rows, Cout], token-major.  w_packed = packing.pack_vitdec_head_train(...)["w"]."""
    M, Mo = _vitdec_head_rows(layer, NV, H, W)
    cout = 1
    if layer in _VITDEC_CONV:
        cin, cout, taps, classes = _VITDEC_CONV[layer]
        _vitdec_packed(x_packed, M, cin, "x_packed")
        want = classes * taps * cin * ((cout + 127) // 128 * 128) * 2
        if w_packed.dtype != torch.bfloat16 or w_packed.numel() != want or not w_packed.is_contiguous():
            raise ValueError("w_packed must hold %d bf16 elements (packing.pack_vitdec_head_train); got %s %d" % (want, w_packed.dtype, w_packed.numel()))
    z = torch.empty(Mo, cout, dtype=torch.float32, device=x_packed.device)
    lib().mvs_vitdec_head_conv_fwd(ptr(x_packed), ptr(w_packed), ptr(z), int(layer), NV, H, W, stream_of(x_packed))
    return z


def vitdec_head_dgrad(dz_packed: torch.Tensor, wt_packed: torch.Tensor, layer: int, NV: int, H: int, W: int) -> torch.Tensor:
    """Data gradient of a head layer: the packed-split d_z of the layer's output map -> fp32 [NV H W, Cin].  wt_packed =
    packing.pack_vitdec_head_train(...)["wT"] (proj: flipped, channel-transposed taps; upsamplers: the 4x4 stride-2 window)."""
    M, Mo = _vitdec_head_rows(layer, NV, H, W)
    cin = 1
    if layer in _VITDEC_CONV:
        cin, cout = _VITDEC_CONV[layer][:2]
        _vitdec_packed(dz_packed, Mo, cout, "dz_packed")
        want = (9 if layer == VITDEC_PROJ else 16) * cout * cin * 2
        if wt_packed.dtype != torch.bfloat16 or wt_packed.numel() != want or not wt_packed.is_contiguous():
            raise ValueError("wt_packed must hold %d bf16 elements (packing.pack_vitdec_head_train); got %s %d" % (want, wt_packed.dtype, wt_packed.numel()))
    d_x = torch.empty(M, cin, dtype=torch.float32, device=dz_packed.device)
    lib().mvs_vitdec_head_dgrad(ptr(dz_packed), ptr(wt_packed), ptr(d_x), int(layer), NV, H, W, stream_of(dz_packed))
    return d_x


def vitdec_head_wgrad_slabs(layer: int, NV: int, H: int, W: int) -> int:
    """Token slabs of vitdec_head_wgrad's launch; 0 = not built (read off the workspace size, as vitdec_wgrad_slabs)."""
    if layer not in _VITDEC_CONV:
        return 0
    cin, cout = _VITDEC_CONV[layer][:2]
    return lib().mvs_vitdec_head_wgrad_workspace_bytes(int(layer), NV, H, W) // ((9 if layer == VITDEC_PROJ else 16) * cin * cout * 4)


def vitdec_head_wgrad(d_z: torch.Tensor, x: torch.Tensor, layer: int, NV: int, H: int, W: int) -> torch.Tensor:
    """Weight gradient of a head layer in the nn layout: d_z fp32 [output rows, Cout], x fp32 [NV H W, Cin] -> proj [256, 768, 3, 3],
    upsamplers [Cin, Cout, 4, 4].  Per-slab partials added in slab order: no atomics."""
    M, Mo = _vitdec_head_rows(layer, NV, H, W)
    cin, cout = _VITDEC_CONV[layer][:2] if layer in _VITDEC_CONV else (None, None)
    _vitdec_tokens(d_z, cout, "d_z")
    _vitdec_tokens(x, cin, "x")
    if layer in _VITDEC_CONV and (d_z.shape[0] != Mo or x.shape[0] != M or x.device != d_z.device):
        raise ValueError("d_z %s and x %s must have %d and %d rows on one device" % (tuple(d_z.shape), tuple(x.shape), Mo, M))
    L = lib()
    ws_bytes = L.mvs_vitdec_head_wgrad_workspace_bytes(int(layer), NV, H, W) if layer in _VITDEC_CONV else 0
    ws = _workspace(ws_bytes, d_z.device)
    if layer == VITDEC_PROJ:
        dw = torch.empty(256, 9 * 768, dtype=torch.float32, device=d_z.device)
    else:
        dw = torch.empty(16 * (cout or 1), cin or 1, dtype=torch.float32, device=d_z.device)
    L.mvs_vitdec_head_wgrad(ptr(d_z), ptr(x), ptr(dw), ptr(ws), ws_bytes, int(layer), NV, H, W, stream_of(d_z))
    if layer == VITDEC_PROJ:
        return dw.view(256, 3, 3, 768).permute(0, 3, 1, 2).contiguous()
    return dw.view(4, 4, cout, cin).permute(3, 2, 0, 1).contiguous()


def vitdec_head_bn_fwd(z: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, conv_bias: Optional[torch.Tensor] = None,
                       running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None, momentum: float = 0.0, *,
                       want_y: bool = True, want_packed: bool = False, planar: Optional[Tuple[int, int, int]] = None):
    """Batch-statistics BatchNorm + SiLU of token-major z fp32 [M, C] (C = 256 | 128 | 64) -> (y, y_packed, stats [3, C] = mean | biased
    variance | invstd).  y is fp32 [M, C] (want_y) and / or packed-split (want_packed); with planar = (NV, H, W), M = NV H W, y is the
    planar fp32 [NV, C, H, W] alone.  running_mean / running_var (updated in place, on the device) take one step of `momentum` with
    mean + conv_bias and the unbiased variance.  Sums in fp64, fixed order."""
    _vitdec_tokens(z, None, "z")
    M, C = z.shape
    for t, what in ((gamma, "gamma"), (beta, "beta")):
        _vitdec_vec(t, C, what, z)
    for t, what in ((conv_bias, "conv_bias"), (running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None:
            _vitdec_vec(t, C, what, z)
    L = lib()
    nbytes = L.mvs_vitdec_head_bn_workspace_bytes(M, C)
    ws = _workspace(nbytes, z.device, unbuilt="mvs_vitdec_head_bn_fwd (rows of %d channels)" % C)
    stats = torch.empty(3, C, dtype=torch.float32, device=z.device)
    y = yp = ypl = None
    pixels = 1
    if planar is not None:
        NV, H, W = planar
        if NV * H * W != M:
            raise ValueError("planar = (NV, H, W) must have NV H W = %d rows; got %s" % (M, planar))
        ypl = torch.empty(NV, C, H, W, dtype=torch.float32, device=z.device)
        pixels = H * W
    else:
        y = torch.empty_like(z) if want_y else None
        yp = torch.empty(L.mvs_vitdec_packed_bytes(M, C), dtype=torch.uint8, device=z.device) if want_packed else None
    L.mvs_vitdec_head_bn_fwd(ptr(z), ptr(conv_bias), ptr(gamma), ptr(beta), float(eps), float(momentum), ptr(running_mean), ptr(running_var),
                             ptr(stats), ptr(y), ptr(yp), ptr(ypl), ptr(ws), nbytes, M, C, pixels, stream_of(z))
    return (ypl if planar is not None else y), yp, stats


def vitdec_head_bn_bwd(d_y: torch.Tensor, z: torch.Tensor, stats: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor):
    """Backward of vitdec_head_bn_fwd: d_y fp32 [M, C] token-major, or the planar [NV, C, H, W] cotangent of the planar form ->
    (d_z fp32 [M, C], d_z packed-split, d_gamma, d_beta)."""
    _vitdec_tokens(z, None, "z")
    M, C = z.shape
    planar = d_y.dim() == 4
    if d_y.dtype != torch.float32 or not d_y.is_contiguous() or d_y.device != z.device or \
            (planar and (d_y.shape[1] != C or d_y.shape[0] * d_y.shape[2] * d_y.shape[3] != M)) or (not planar and d_y.shape != z.shape):
        raise ValueError("d_y must be contiguous fp32 %s or planar [NV, %d, H, W] with NV H W = %d; got %s %s" % (tuple(z.shape), C, M, d_y.dtype, tuple(d_y.shape)))
    if stats.dtype != torch.float32 or tuple(stats.shape) != (3, C) or not stats.is_contiguous():
        raise ValueError("stats must be vitdec_head_bn_fwd's fp32 [3, %d]" % C)
    _vitdec_vec(gamma, C, "gamma", z)
    _vitdec_vec(beta, C, "beta", z)
    L = lib()
    nbytes = L.mvs_vitdec_head_bn_workspace_bytes(M, C)
    ws = _workspace(nbytes, z.device, unbuilt="mvs_vitdec_head_bn_bwd (rows of %d channels)" % C)
    d_z = torch.empty_like(z)
    d_zp = torch.empty(L.mvs_vitdec_packed_bytes(M, C), dtype=torch.uint8, device=z.device)
    d_gb = torch.empty(2, C, dtype=torch.float32, device=z.device)
    L.mvs_vitdec_head_bn_bwd(ptr(d_y), int(planar), ptr(z), ptr(stats), ptr(gamma), ptr(beta), ptr(d_z), ptr(d_zp), ptr(d_gb), ptr(ws), nbytes,
                             M, C, d_y.shape[2] * d_y.shape[3] if planar else 1, stream_of(z))
    return d_z, d_zp, d_gb[0], d_gb[1]


VIT_KEY_STEP = 32          # the attention core's key step: every view's rows are padded to a multiple of it
VIT_KPAD = 640             # the patch embedding's K = 588 padded to the GEMM's chunk


def vit_npad(ntok: int) -> int:
    """Rows per view of the ViT's working buffers: ntok = n + 1 tokens rounded up to a multiple of 32."""
    return (int(ntok) + VIT_KEY_STEP - 1) // VIT_KEY_STEP * VIT_KEY_STEP


def vit_rows(x: torch.Tensor, *, ln: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, eps: float = 1e-6,
             norm: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """Row pass of the ViT backbone on the residual stream x fp32 contiguous [M, 768]: ln -> packed-split LayerNorm(ln, eps)(x) (the row
    operand of qkv / fc1); norm -> fp32 [M, 768] LayerNorm(norm, eps 1e-6)(x) (the final norm).  Returns (normed or None, packed or None)."""
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 768 or not x.is_contiguous():
        raise ValueError("vit_rows takes the residual stream: contiguous fp32 [M, 768]; got %s %s" % (x.dtype, tuple(x.shape)))
    if (ln is None) == (norm is None):
        raise ValueError("vit_rows: give exactly one of ln (packed-split output) and norm (fp32 output)")
    for pair, what in ((ln, "ln"), (norm, "norm")):
        if pair is not None:
            _vitdec_vec(pair[0], 768, what + " weight", x)
            _vitdec_vec(pair[1], 768, what + " bias", x)
    M = x.shape[0]
    L = lib()
    y = torch.empty_like(x) if norm is not None else None
    xn = torch.empty(L.mvs_vitdec_packed_bytes(M, 768), dtype=torch.uint8, device=x.device) if ln is not None else None
    L.mvs_vit_rows_fwd(ptr(x), 0, M * 768, M * 768, 768, 0, 1, None, None, ptr(norm[0]) if norm else None, ptr(norm[1]) if norm else None, ptr(y),
                       None, 1, 0, ptr(ln[0]) if ln else None, ptr(ln[1]) if ln else None, float(eps), ptr(xn), 1, M, 768, stream_of(x))
    return y, xn


def vit_patches(img: torch.Tensor) -> torch.Tensor:
    """img [NV, 3, 14 gh, 14 gw] (fp32 / bf16 / fp16, ANY strides: read in place) -> the packed-split [NV gh gw, 640] row operand of the
    patch embedding (column c * 196 + ky * 14 + kx, zero past 588)."""
    if img.dim() != 4 or img.shape[1] != 3 or img.dtype not in _lib.DTYPE_CODE or img.shape[2] % 14 or img.shape[3] % 14 or min(img.shape) < 1 \
            or min(img.stride()) < 0:
        raise ValueError("vit_patches takes an image [NV, 3, H, W] fp32 / bf16 / fp16 with H and W multiples of 14; got %s %s"
                         % (img.dtype, tuple(img.shape)))
    NV, _, H, W = img.shape
    gh, gw = H // 14, W // 14
    out = torch.empty(lib().mvs_vitdec_packed_bytes(NV * gh * gw, VIT_KPAD), dtype=torch.uint8, device=img.device)
    lib().mvs_vit_patches_fwd(_base_ptr(img), _lib.DTYPE_CODE[img.dtype], img.stride(0), img.stride(1), img.stride(2), img.stride(3),
                              ptr(out), NV, gh, gw, 14, 3, stream_of(img))
    return out


def vit_embed(a_packed: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, pos: torch.Tensor, cls_pos: torch.Tensor, NV: int,
              n: int) -> torch.Tensor:
    """The ViT's tokens: fp32 [NV * npad, 768] with npad = vit_npad(n + 1): per view row 0 = cls_pos, rows 1 .. n = patches W^T + bias +
    pos[1 + patch], the rest zero.  (w_packed, bias) = packing.pack_vit_patch_embed, pos = packing.vit_position_table [n + 1, 768],
    cls_pos = cls_token + pos[0]."""
    _vitdec_packed(a_packed, NV * n, VIT_KPAD, "a_packed")
    if w_packed.dtype != torch.bfloat16 or w_packed.numel() != 2 * VIT_KPAD * 768 or not w_packed.is_contiguous():
        raise ValueError("w_packed must come from packing.pack_vit_patch_embed: %d bf16 elements, got %s %d"
                         % (2 * VIT_KPAD * 768, w_packed.dtype, w_packed.numel()))
    _vitdec_vec(bias, 768, "bias", a_packed)
    _vitdec_vec(pos, (n + 1) * 768, "pos", a_packed)
    _vitdec_vec(cls_pos, 768, "cls_pos", a_packed)
    npad = vit_npad(n + 1)
    x = torch.empty(NV * npad, 768, dtype=torch.float32, device=a_packed.device)
    lib().mvs_vit_embed_fwd(ptr(a_packed), ptr(w_packed), ptr(bias), ptr(pos), ptr(cls_pos), ptr(x), int(NV), int(n), npad, 768, stream_of(a_packed))
    return x


def vit_qkv(xn_packed: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, NV: int, npad: int, q_scale: float) -> torch.Tensor:
    """The attention core's operands (uint8, mvs_vit_qkv_bytes(NV, npad)) from xn packed-split [NV * npad, 768]: q * q_scale | k per head
    as packed-split rows, v transposed.  w_packed = pack_linear_bf16x3(qkv.weight [2304, 768]); q_scale = softmax scale * log2(e)."""
    if npad < VIT_KEY_STEP or npad % VIT_KEY_STEP:
        raise ValueError("npad must be a multiple of %d (ops.vit_npad); got %d" % (VIT_KEY_STEP, npad))
    _vitdec_packed(xn_packed, NV * npad, 768, "xn_packed")
    if w_packed.dtype != torch.bfloat16 or w_packed.numel() != 2 * 768 * 2304 or not w_packed.is_contiguous():
        raise ValueError("w_packed must come from packing.pack_linear_bf16x3(qkv.weight [2304, 768]): %d bf16 elements, got %s %d"
                         % (2 * 768 * 2304, w_packed.dtype, w_packed.numel()))
    _vitdec_vec(bias, 2304, "bias", xn_packed)
    out = torch.empty(lib().mvs_vit_qkv_bytes(NV, npad), dtype=torch.uint8, device=xn_packed.device)
    lib().mvs_vit_qkv_fwd(ptr(xn_packed), ptr(w_packed), ptr(bias), ptr(out), int(NV), int(npad), float(q_scale), 768, stream_of(xn_packed))
    return out


def vit_attention(qkv: torch.Tensor, NV: int, ntok: int, npad: int, heads: int = 12, head_dim: int = 64) -> torch.Tensor:
    """softmax(q k^T) v over the ntok tokens of each view and head (q pre-scaled, scores in log2 units) -> packed-split [NV * npad, 768]."""
    if npad < VIT_KEY_STEP or npad % VIT_KEY_STEP or not 1 <= ntok <= npad:
        raise ValueError("vit_attention: 1 <= ntok <= npad, npad a multiple of %d; got ntok %d, npad %d" % (VIT_KEY_STEP, ntok, npad))
    want = lib().mvs_vit_qkv_bytes(NV, npad)
    if qkv.dtype != torch.uint8 or qkv.dim() != 1 or qkv.numel() != want or not qkv.is_contiguous():
        raise ValueError("qkv must be vit_qkv's uint8 tensor of mvs_vit_qkv_bytes(%d, %d) = %d bytes; got %s %s"
                         % (NV, npad, want, qkv.dtype, tuple(qkv.shape)))
    out = torch.empty(lib().mvs_vitdec_packed_bytes(NV * npad, 768), dtype=torch.uint8, device=qkv.device)
    lib().mvs_vit_attention_fwd(ptr(qkv), ptr(out), int(NV), int(ntok), int(npad), int(heads), int(head_dim), stream_of(qkv))
    return out


def _feat(t) -> Tuple[torch.Tensor, int]:
    if isinstance(t, PackedFeatures):
        return t, _lib.DTYPE_CODE[t.dtype]
    if t.dtype not in _lib.DTYPE_CODE:
        t = t.float()
    return t.contiguous(), _lib.DTYPE_CODE[t.dtype]


def _feat_ptr(features):
    """(tensor handed to the C ABI, layout code)"""
    if isinstance(features, PackedFeatures):
        return features.data, _lib.LAYOUT_OCTET_TILED
    return features, _lib.LAYOUT_PLANAR


# ---- a1 + warping.py:80 -------------------------------------------------------------------------
def compose_homography(proj_matrices: torch.Tensor) -> torch.Tensor:
    """proj_matrices [B,V,2,4,4] -> per-source-view homographies [B,V-1,12] (R row-major, then t)."""
    p = _f32c(proj_matrices)
    B, V = p.shape[:2]
    assert p.shape[2:] == (2, 4, 4), "proj_matrices must be [B,V,2,4,4]"
    out = torch.empty(B, V - 1, 12, dtype=torch.float32, device=p.device)
    lib().mvs_compose_homography(ptr(p), B, V, ptr(out), stream_of(p))
    return out


def cascade_prologue(proj_matrices: Sequence[torch.Tensor], depth_values: Optional[torch.Tensor] = None, ndepths: int = 0, H: int = 0, W: int = 0,
                     inverse: bool = True):
    """Round 5: the cascade's prologue in ONE launch (mvs_cascade_prologue_fwd): the homographies of every stage's proj_matrices
    [B,V,2,4,4] -> list of [B,V-1,12], and - depth_values [B,N] given - stage 1's hypotheses [B,ndepths,H,W] (init_range)."""
    ps = [_f32c(p) for p in proj_matrices]
    B, V = ps[0].shape[:2]
    for p in ps:
        assert p.shape == (B, V, 2, 4, 4), "proj_matrices must be [B,V,2,4,4] with the same B, V on every stage"
    hom = torch.empty(len(ps), B, V - 1, 12, dtype=torch.float32, device=ps[0].device)
    hyp, dv, N = None, None, 0
    if depth_values is not None:
        dv = _f32c(depth_values)
        assert dv.dim() == 2 and dv.shape[0] == B, "depth_values must be [B,N] (per-pixel ranges go through init_range)"
        N = dv.shape[1]
        hyp = torch.empty(B, ndepths, H, W, dtype=torch.float32, device=dv.device)
    pa = _ptr_array(ps)
    lib().mvs_cascade_prologue_fwd(C.cast(pa, C.c_void_p), len(ps), B, V, ptr(hom), ptr(dv), N, 1 if inverse else 0, ptr(hyp), ndepths, H, W,
                                   stream_of(ps[0]))
    return list(hom.unbind(0)), hyp


def homography_from_proj(src_proj: torch.Tensor, ref_proj: torch.Tensor) -> torch.Tensor:
    s, r = _f32c(src_proj), _f32c(ref_proj)
    B = s.shape[0]
    out = torch.empty(B, 12, dtype=torch.float32, device=s.device)
    lib().mvs_homography_from_proj(ptr(s), ptr(r), B, ptr(out), stream_of(s))
    return out


def homo_warp(src_fea: torch.Tensor, homography: torch.Tensor, depth_values: torch.Tensor,
              want_warped: bool = True, want_mask: bool = True):
    f, code = _feat(src_fea)
    B, Cc, H, W = f.shape
    dv = _f32c(depth_values)
    D = dv.shape[1]
    is_vol = 1 if dv.dim() == 4 else 0
    warped = torch.empty(B, Cc, D, H, W, dtype=torch.float32, device=f.device) if want_warped else None
    mask = torch.empty(B, D, H, W, dtype=torch.uint8, device=f.device) if want_mask else None
    lib().mvs_homo_warp_fwd(ptr(f), code, ptr(homography.contiguous()), ptr(dv), is_vol, ptr(warped), ptr(mask), B, Cc, D, H, W, stream_of(f))
    return warped, (mask.bool() if mask is not None else None)


# ---- a2-a6 --------------------------------------------------------------------------------------
def warp_corr_entropy(features: torch.Tensor, code: int, homography: torch.Tensor, hyp: torch.Tensor, G: int,
                      view_begin: int = 1, view_end: Optional[int] = None, out: Optional[torch.Tensor] = None, f16_window: bool = False) -> torch.Tensor:
    """features [B,V,C,H,W] contiguous; -> entropy [B,V-1,H,W] (only views in [view_begin, view_end) are written; pass a
    preallocated `out` to skip the zero fill when every view is written).  f16_window: MVS_GATHER_F16 (the fp16 formats' gather:
    source window staged as fp16)."""
    B, V, Cc, H, W = features.shape
    D = hyp.shape[1]
    view_end = V if view_end is None else view_end
    if out is not None:
        ent = out
    elif view_begin == 1 and view_end == V:
        ent = torch.empty(B, V - 1, H, W, dtype=torch.float32, device=features.device)
    else:
        ent = torch.zeros(B, V - 1, H, W, dtype=torch.float32, device=features.device)
    ft, layout = _feat_ptr(features)
    lib().mvs_warp_corr_entropy_fwd(ptr(ft), code, layout, ptr(homography), ptr(hyp), ptr(ent), B, V, Cc, G, D, H, W,
                                    view_begin, view_end, 1 if f16_window else 0, stream_of(ft))
    return ent


def vis_weight(entropy: torch.Tensor, params: Sequence[torch.Tensor], precision: int = 0) -> torch.Tensor:
    """entropy [..., H, W] -> sigmoid(vis CNN) of the same shape.  params = packed (w1,b1,w2,b2,w3,b3,w4,b4)."""
    e = _f32c(entropy)
    H, W = e.shape[-2:]
    N = e.numel() // (H * W)
    vis = torch.empty_like(e)
    nbytes = lib().mvs_vis_workspace_bytes(N, H, W, precision)
    ws = _workspace(nbytes, e.device)
    lib().mvs_vis_weight_fwd(ptr(e), *[ptr(p) for p in params], ptr(vis), ptr(ws), nbytes, N, H, W, precision, stream_of(e))
    return vis


def vis_conv1(entropy: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor) -> torch.Tensor:
    e = _f32c(entropy)
    H, W = e.shape[-2:]
    N = e.numel() // (H * W)
    out = torch.empty(N, H, W, 16, dtype=torch.float32, device=e.device)
    lib().mvs_vis_conv1_fwd(ptr(e), ptr(w1), ptr(b1), ptr(out), N, H, W, stream_of(e))
    return out


def vis_out(x_cl8: torch.Tensor, w4: torch.Tensor, b4: torch.Tensor, shape) -> torch.Tensor:
    N, H, W, _ = x_cl8.shape
    vis = torch.empty(shape, dtype=torch.float32, device=x_cl8.device)
    lib().mvs_vis_out_fwd(ptr(x_cl8), ptr(w4), ptr(b4), ptr(vis), N, H, W, stream_of(x_cl8))
    return vis


def warp_corr_aggregate(features: torch.Tensor, code: int, homography: torch.Tensor, hyp: torch.Tensor, vis: torch.Tensor,
                        G: int, normalise: bool = True, view_begin: int = 1, view_end: Optional[int] = None, out=None, split: bool = False,
                        f16: bool = False):
    """-> (volume_cl [B,D,H,W,G], vis_sum [B,H,W] or None).  `out` = preallocated (volume, vis_sum) to fill.
    split: leave the (normalised, G = 8) volume in the split activation format of the bf16x3 U-Net (to_split / from_split);
    f16: write it as fp16 (the cost volume of the MVS_PREC_F16X2 U-Net; LDS-staged gather shapes only)."""
    B, V, Cc, H, W = features.shape
    D = hyp.shape[1]
    view_end = V if view_end is None else view_end
    if out is not None:
        vol, vsum = out
    else:
        vol = torch.empty(B, D, H, W, G, dtype=torch.float16 if f16 else torch.float32, device=features.device)
        vsum = None if normalise else torch.empty(B, H, W, dtype=torch.float32, device=features.device)
    ft, layout = _feat_ptr(features)
    lib().mvs_warp_corr_aggregate_fwd(ptr(ft), code, layout, ptr(homography), ptr(hyp), ptr(vis), ptr(vol), ptr(vsum),
                                      1 if normalise else 0, _lib.VOLUME_F16 if f16 else (_lib.VOLUME_SPLIT if split else _lib.VOLUME_F32), B, V, Cc, G, D, H, W,
                                      view_begin, view_end, stream_of(ft))
    return vol, vsum


def warp_corr_aggregate_bwd(features: torch.Tensor, code: int, homography: torch.Tensor, hyp: torch.Tensor, vis: torch.Tensor,
                            vis_sum: torch.Tensor, volume_cl: torch.Tensor, grad_volume_cl: torch.Tensor, G: int):
    """Backward of warp_corr_aggregate(normalise=True) -> (grad_features [B,V,C,H,W] fp32, grad_vis [B,V-1,H,W])."""
    B, V, Cc, H, W = features.shape
    D = hyp.shape[1]
    gfeat = torch.empty(B, V, Cc, H, W, dtype=torch.float32, device=features.device)
    gvis = torch.empty(B, V - 1, H, W, dtype=torch.float32, device=features.device)
    lib().mvs_warp_corr_aggregate_bwd(ptr(features), code, ptr(homography), ptr(hyp), ptr(vis), ptr(vis_sum), ptr(volume_cl),
                                      ptr(grad_volume_cl), ptr(gfeat), ptr(gvis), B, V, Cc, G, D, H, W, stream_of(features))
    return gfeat, gvis


def volume_normalise_(vol_cl: torch.Tensor, vis_sum: torch.Tensor, split: bool = False) -> torch.Tensor:
    B, D, H, W, G = vol_cl.shape
    lib().mvs_volume_normalise(ptr(vol_cl), ptr(vis_sum), B, D, H, W, G, _lib.VOLUME_SPLIT if split else _lib.VOLUME_F32, stream_of(vol_cl))
    return vol_cl


def gather_is_lds_staged(features, G: int, hyp: torch.Tensor) -> bool:
    """Do the gather passes take the LDS-staged kernels for this call (they alone write the split / fp16 volume directly)?"""
    B, V, Cc, H, W = features.shape
    _, layout = _feat_ptr(features)
    return bool(lib().mvs_gather_is_lds_staged(layout, Cc, G, hyp.shape[1], H, W))


def gather_keeps_correlations(features, G: int, hyp: torch.Tensor) -> bool:
    """Is the correlation-keeping pass 1 (warp_corr_entropy_keep + corr_aggregate) built for this call's shapes?"""
    B, V, Cc, H, W = features.shape
    _, layout = _feat_ptr(features)
    return bool(lib().mvs_gather_keeps_correlations(layout, Cc, G, hyp.shape[1], H, W))


def warp_corr_entropy_keep(features, code: int, homography: torch.Tensor, hyp: torch.Tensor, G: int, exact: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Pass 1 over all source views that also KEEPS the per-view group correlations (cost_volume.py:79-84):
    -> (entropy [B,V-1,H,W] fp32, corr [B,V-1,D,H,W,8]).  corr is fp16 from fp16 source windows (MVS_CORR_F16), or - `exact` - fp32 from
    fp32 windows (MVS_CORR_F32): corr_aggregate then writes what the second gather would have."""
    B, V, Cc, H, W = features.shape
    D = hyp.shape[1]
    ft, layout = _feat_ptr(features)
    ent = torch.empty(B, V - 1, H, W, dtype=torch.float32, device=ft.device)
    corr = torch.empty(B, V - 1, D, H, W, 8, dtype=torch.float32 if exact else torch.float16, device=ft.device)
    lib().mvs_warp_corr_entropy_keep_fwd(ptr(ft), code, layout, ptr(homography), ptr(hyp), ptr(ent), ptr(corr),
                                         _lib.CORR_F32 if exact else _lib.CORR_F16, B, V, Cc, G, D, H, W, stream_of(ft))
    return ent, corr


def corr_aggregate(corr: torch.Tensor, vis: torch.Tensor, split: bool = False, f16: bool = True) -> torch.Tensor:
    """corr [B,V-1,D,H,W,8] fp16 or fp32 (warp_corr_entropy_keep), vis [B,V-1,H,W] fp32 -> the normalised cost volume [B,D,H,W,8]
    (cost_volume.py:97-101): fp16 (f16, the fp16 U-Nets' format), the split activation format of the bf16x3 U-Net (split) or fp32
    (neither; the transformer regulariser)."""
    assert corr.dtype in (torch.float16, torch.float32) and corr.is_contiguous() and corr.dim() == 6 and corr.shape[-1] == 8
    B, NV, D, H, W, _ = corr.shape
    v = _f32c(vis)
    assert v.shape == (B, NV, H, W)
    f16 = f16 and not split
    vol = torch.empty(B, D, H, W, 8, dtype=torch.float16 if f16 else torch.float32, device=corr.device)
    fmt = _lib.VOLUME_F16 if f16 else (_lib.VOLUME_SPLIT if split else _lib.VOLUME_F32)
    cfmt = _lib.CORR_F32 if corr.dtype == torch.float32 else _lib.CORR_F16
    lib().mvs_corr_aggregate_fwd(ptr(corr), cfmt, ptr(v), ptr(vol), fmt, B, NV + 1, D, H, W, stream_of(corr))
    return vol


def f16_saturation_count(reset: bool = False, device=None) -> int:
    """Work-items that stored an fp16 ACTIVATION beyond +-65504 (clamped) on `device` (default: the current one) since the last reset -
    0 unless the "f16x2" format degraded something the fp32-equivalent "bf16x3" would have kept.  Synchronises the device."""
    if device is not None and torch.device(device).type == "cuda":
        with torch.cuda.device(device):
            return int(lib().mvs_f16_saturation_count(1 if reset else 0))
    return int(lib().mvs_f16_saturation_count(1 if reset else 0))


def volume_to_f16(vol_cl: torch.Tensor, vis_sum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 volume [B,D,H,W,8] (divided by vis_sum + 1e-6 first when given) -> fp16 in a new buffer, clamped to the fp16 range."""
    B, D, H, W, G = vol_cl.shape
    out = torch.empty(B, D, H, W, G, dtype=torch.float16, device=vol_cl.device)
    lib().mvs_volume_to_f16(ptr(vol_cl), ptr(vis_sum), ptr(out), B, D, H, W, G, stream_of(vol_cl))
    return out


def slab_pack(vol_cl: torch.Tensor, vis_sum: torch.Tensor, send_bufs, rows) -> None:
    """One launch: send_bufs[j] (or None) <- rows[j] = [r0, r1) of the partial volume [B,D,H,W,G] followed by the same rows of the
    partial visibility sum [B,H,W] (the messages of the slab exchange)."""
    import ctypes as C
    B, D, H, W, G = vol_cl.shape
    n = len(send_bufs)
    fn = lib().mvs_slab_pack          # FIRST: fetching the entry point clears the per-call device record that ptr() fills
    ptrs = (C.c_void_p * n)(*[None if b is None else ptr(b) for b in send_bufs])
    r0 = (C.c_int * n)(*[int(r[0]) for r in rows])
    r1 = (C.c_int * n)(*[int(r[1]) for r in rows])
    fn(ptr(vol_cl), ptr(vis_sum), C.cast(ptrs, C.c_void_p), C.cast(r0, C.c_void_p), C.cast(r1, C.c_void_p), n, B, D, H, W, G, stream_of(vol_cl))


def slab_reduce(vol_cl: torch.Tensor, vis_sum: torch.Tensor, recv_bufs, my_rank: int, out: torch.Tensor, r0: int, r1: int) -> torch.Tensor:
    """One launch: out <- sum over ranks, in rank order, of their partials of rows [r0, r1): the own slice read in place, the others
    from recv_bufs[j] (None = rank j sent nothing)."""
    import ctypes as C
    B, D, H, W, G = vol_cl.shape
    n = len(recv_bufs)
    fn = lib().mvs_slab_reduce        # before the pointer array, see slab_pack
    ptrs = (C.c_void_p * n)(*[None if b is None else ptr(b) for b in recv_bufs])
    fn(ptr(vol_cl), ptr(vis_sum), C.cast(ptrs, C.c_void_p), n, my_rank, ptr(out), r0, r1, B, D, H, W, G, stream_of(vol_cl))
    return out


def to_split(x_cl: torch.Tensor) -> torch.Tensor:
    """fp32 channel-last [..., C] -> the split activation format of MVS_PREC_BF16X3_SPLIT, same shape and dtype (the bytes are, per
    voxel, C / 8 octets of [hi x8 | lo x8] bf16 with hi = bf16(x), lo = bf16(x - hi)).  Plain torch ops: a test / tooling utility,
    the product path never converts (the kernels' epilogues write the format)."""
    C = x_cl.shape[-1]
    pair = packing.split_bf16(x_cl.reshape(*x_cl.shape[:-1], C // 8, 8)).movedim(0, -2)                             # [..., C/8, 2, 8]
    return pair.contiguous().view(torch.float32).reshape(x_cl.shape)


def from_split(s_cl: torch.Tensor) -> torch.Tensor:
    """Inverse of to_split up to the split's 2^-17 relative rounding: hi + lo as fp32."""
    C = s_cl.shape[-1]
    pair = s_cl.contiguous().view(torch.bfloat16).reshape(*s_cl.shape[:-1], C // 8, 2, 8).float()
    return (pair[..., 0, :] + pair[..., 1, :]).reshape(s_cl.shape)


# ---- a7-a9 --------------------------------------------------------------------------------------
def _act_dtype(x_cl: torch.Tensor, precision: int):
    """Element type of the activation tensors of a call: fp16 for MVS_PREC_F16X2, fp32 (plain or split pairs) otherwise."""
    want = torch.float16 if precision in _lib.F16_CODES else torch.float32
    if x_cl.dtype != want:
        raise _lib.MvsHipError("precision %d takes %s activations, got %s" % (precision, want, x_cl.dtype))
    return want


def conv3d_bn_relu(x_cl: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, cout: int, kd: int,
                   stride: Tuple[int, int, int], relu: bool = True, precision: int = 0) -> torch.Tensor:
    B, D, H, W, cin = x_cl.shape
    sd, sh, sw = stride
    pd = kd // 2
    od, oh, ow = (D + 2 * pd - kd) // sd + 1, (H - 1) // sh + 1, (W - 1) // sw + 1
    y = torch.empty(B, od, oh, ow, cout, dtype=_act_dtype(x_cl, precision), device=x_cl.device)
    lib().mvs_conv3d_bn_relu_fwd(ptr(x_cl), ptr(w_packed), ptr(bias), ptr(y), B, cin, cout, D, H, W, kd, sd, sh, sw,
                                 1 if relu else 0, precision, stream_of(x_cl))
    return y


def deconv3d_bn_relu_add(x_cl: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, cout: int, sd: int,
                         skip_cl: Optional[torch.Tensor] = None, precision: int = 0) -> torch.Tensor:
    B, D, H, W, cin = x_cl.shape
    y = torch.empty(B, D * sd, 2 * H, 2 * W, cout, dtype=_act_dtype(x_cl, precision), device=x_cl.device)
    if skip_cl is not None:
        assert tuple(skip_cl.shape) == tuple(y.shape) and skip_cl.dtype == y.dtype, "skip tensor shape / dtype mismatch"
    lib().mvs_deconv3d_bn_relu_add_fwd(ptr(x_cl), ptr(w_packed), ptr(bias), ptr(skip_cl), ptr(y), B, cin, cout, D, H, W,
                                       sd, precision, stream_of(x_cl))
    return y


def conv3d_is_tuned(cin: int, cout: int, kd: int, stride: Tuple[int, int, int]) -> bool:
    """A tuned MFMA kernel exists for Conv3d(cin, cout, (kd,3,3), stride, padding (kd//2,1,1)) (the table of csrc/conv_cfg.h)."""
    return bool(lib().mvs_conv3d_is_tuned(cin, cout, kd, *stride))


def deconv3d_is_tuned(cin: int, cout: int, sd: int) -> bool:
    return bool(lib().mvs_deconv3d_is_tuned(cin, cout, sd))


def conv3d_generic(x_cl: torch.Tensor, w_tck: torch.Tensor, bias: Optional[torch.Tensor], cout: int, ksize: Tuple[int, int, int],
                   stride: Tuple[int, int, int], padding: Tuple[int, int, int], relu: bool = False, skip_cl: Optional[torch.Tensor] = None,
                   transposed: bool = False, output_padding: Tuple[int, int, int] = (0, 0, 0)) -> torch.Tensor:
    """Shape-generic exact-fp32 Conv3d / ConvTranspose3d + bias + ReLU + skip (mvs_conv3d_generic_fwd): x_cl [B,D,H,W,Cin] fp32 ->
    [B,OD,OH,OW,cout] fp32; w_tck = packing.pack_generic_conv_weights / pack_generic_deconv_weights ([taps][Cin][Cout])."""
    if x_cl.dtype != torch.float32:
        raise _lib.MvsHipError("the generic convolution takes fp32 activations, got %s" % x_cl.dtype)
    B, D, H, W, cin = x_cl.shape
    k, s, p = tuple(ksize), tuple(stride), tuple(padding)
    if tuple(w_tck.shape) != (k[0] * k[1] * k[2], cin, cout) or w_tck.dtype != torch.float32:
        raise _lib.MvsHipError("generic convolution weights %s %s do not match fp32 [%d][%d][%d]" % (tuple(w_tck.shape), w_tck.dtype, k[0] * k[1] * k[2], cin, cout))
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() < cout):
        raise _lib.MvsHipError("generic convolution bias must be fp32 with at least %d entries, got %s %s" % (cout, bias.dtype, tuple(bias.shape)))
    if transposed:
        out = [(n - 1) * s[i] - 2 * p[i] + k[i] + output_padding[i] for i, n in enumerate((D, H, W))]
    else:
        out = [(n + 2 * p[i] - k[i]) // s[i] + 1 for i, n in enumerate((D, H, W))]
    y = torch.empty(B, out[0], out[1], out[2], cout, dtype=torch.float32, device=x_cl.device)
    if skip_cl is not None and (tuple(skip_cl.shape) != tuple(y.shape) or skip_cl.dtype != torch.float32):
        raise _lib.MvsHipError("skip tensor %s / %s does not match the layer output %s fp32" % (tuple(skip_cl.shape), skip_cl.dtype, tuple(y.shape)))
    lib().mvs_conv3d_generic_fwd(ptr(x_cl), ptr(w_tck), ptr(bias), ptr(skip_cl), ptr(y), B, cin, cout, D, H, W, out[0], out[1], out[2], k[0], k[1],
                                 k[2], s[0], s[1], s[2], p[0], p[1], p[2], 1 if transposed else 0, 1 if relu else 0, stream_of(x_cl))
    return y


def deconv3d_prob(x_cl: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, sd: int, skip_cl: torch.Tensor, prob_w: torch.Tensor,
                  prob_b: torch.Tensor, precision: int) -> torch.Tensor:
    """Last U-Net layer (Cout = 8) + skip + 1x1x1 `prob` in one launch -> logits [B, D*sd, 2H, 2W]."""
    B, D, H, W, cin = x_cl.shape
    _act_dtype(x_cl, precision)
    _act_dtype(skip_cl, precision)
    logits = torch.empty(B, D * sd, 2 * H, 2 * W, dtype=torch.float32, device=x_cl.device)
    lib().mvs_deconv3d_prob_fwd(ptr(x_cl), ptr(w_packed), ptr(bias), ptr(skip_cl), ptr(prob_w), ptr(prob_b), ptr(logits), B, cin, D, H, W,
                                sd, precision, stream_of(x_cl))
    return logits


# ---- section 8f #2: training-mode regulariser ----------------------------------------------------
def deconv3d_linear(x_cl: torch.Tensor, w_packed: torch.Tensor, zero_bias: torch.Tensor, cout: int, sd: int, precision: int) -> torch.Tensor:
    """ConvTranspose3d(k3, padding 1, stride (sd,2,2), output_padding (sd-1,1,1)) without bias / BatchNorm / ReLU."""
    B, D, H, W, cin = x_cl.shape
    y = torch.empty(B, D * sd, 2 * H, 2 * W, cout, dtype=torch.float32, device=x_cl.device)
    lib().mvs_deconv3d_linear_fwd(ptr(x_cl), ptr(w_packed), ptr(zero_bias), ptr(y), B, cin, cout, D, H, W, sd, precision, stream_of(x_cl))
    return y


def bn_stats(x_cl: torch.Tensor, groups: int = 1) -> torch.Tensor:
    """-> float64 [groups, 2C] (or [2C]): per-channel [sum x | sum x^2] of each of `groups` equal slices along the leading axis."""
    Cc = x_cl.shape[-1]
    sums = torch.empty(groups, 2 * Cc, dtype=torch.float64, device=x_cl.device)
    lib().mvs_bn_stats(ptr(x_cl), ptr(sums), x_cl.numel() // Cc // groups, Cc, groups, stream_of(x_cl))
    return sums if groups > 1 else sums[0]


def bn_finalize(sums: torch.Tensor, count: float, eps: float, running_mean=None, running_var=None, momentum: float = 0.0):
    """-> (mean, biased var, invstd), each [C] or [groups, C]; with running statistics given, their momentum step(s) - one per group,
    in order - happen in the same launch."""
    groups = sums.shape[0] if sums.dim() == 2 else 1
    Cc = sums.shape[-1] // 2
    buf = torch.empty(3, groups, Cc, dtype=torch.float32, device=sums.device)
    lib().mvs_bn_finalize(ptr(sums), float(count), float(eps), ptr(buf[0]), ptr(buf[1]), ptr(buf[2]), ptr(running_mean), ptr(running_var),
                          float(momentum), Cc, groups, stream_of(sums))
    if sums.dim() == 2:
        return buf[0], buf[1], buf[2]
    return buf[0, 0], buf[1, 0], buf[2, 0]


def bn_running_update(mean, var, count: float, momentum: float, running_mean, running_var) -> None:
    groups = mean.shape[0] if mean.dim() == 2 else 1
    lib().mvs_bn_running_update(ptr(mean), ptr(var), float(count), float(momentum), ptr(running_mean), ptr(running_var), mean.shape[-1],
                                groups, stream_of(mean))


def _bn_groups(mean):
    return mean.shape[0] if mean.dim() == 2 else 1


def bn_relu_apply(z_cl, mean, invstd, gamma, beta, skip_cl=None, relu=True) -> torch.Tensor:
    """mean / invstd [C], or [groups, C] for `groups` equal slices of z_cl along its leading axis."""
    Cc, groups = z_cl.shape[-1], _bn_groups(mean)
    y = torch.empty_like(z_cl)
    lib().mvs_bn_relu_apply(ptr(z_cl), ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ptr(skip_cl), ptr(y), z_cl.numel() // Cc // groups, Cc,
                            1 if relu else 0, groups, stream_of(z_cl))
    return y


def bn_relu_bwd_reduce(dy_cl, z_cl, mean, invstd, gamma, beta, relu=True) -> torch.Tensor:
    """-> float64 [2C] (or [groups, 2C]): [sum g | sum g * xhat] with g = dy through the ReLU mask (= [d beta | d gamma] of these voxels)."""
    Cc, groups = z_cl.shape[-1], _bn_groups(mean)
    sums = torch.empty(groups, 2 * Cc, dtype=torch.float64, device=z_cl.device)
    lib().mvs_bn_relu_bwd(ptr(dy_cl), ptr(z_cl), ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ptr(sums), 1.0, None,
                          z_cl.numel() // Cc // groups, Cc, 1 if relu else 0, 1, 0, groups, stream_of(z_cl))
    return sums if mean.dim() == 2 else sums[0]


def bn_relu_bwd_apply(dy_cl, z_cl, mean, invstd, gamma, beta, sums, count: float, relu=True, use_batch_stats=True) -> torch.Tensor:
    Cc, groups = z_cl.shape[-1], _bn_groups(mean)
    dz = torch.empty_like(z_cl)
    lib().mvs_bn_relu_bwd(ptr(dy_cl), ptr(z_cl), ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ptr(sums), float(count), ptr(dz),
                          z_cl.numel() // Cc // groups, Cc, 1 if relu else 0, 1 if use_batch_stats else 0, 1, groups, stream_of(z_cl))
    return dz


class TrainWorkspace:
    """Scratch shared by the block calls of one autograd Function: zero bias, packed-weight buffer, statistics sums."""

    def __init__(self, device):
        self.zero_bias = torch.zeros(64, dtype=torch.float32, device=device)
        self.wpack = torch.empty(64 * 64 * 32 * 2, dtype=torch.bfloat16, device=device)      # >= any packed U-Net weight (64 x 64 x 27, hi + lo)
        self.sums = torch.empty(16 * 2 * 64, dtype=torch.float64, device=device)             # up to 16 statistics groups


def _out_dims(transposed, kd, stride, D, H, W):
    sd, sh, sw = stride
    if transposed:
        return D * sd, 2 * H, 2 * W
    return (D + 2 * (kd // 2) - kd) // sd + 1, (H - 1) // sh + 1, (W - 1) // sw + 1


def train_block_fwd(ws: TrainWorkspace, a_in, w, transposed: bool, kd: int, stride, gamma, beta, eps: float, running_mean, running_var,
                    momentum: float, skip=None, groups: int = 1):
    """conv / transposed conv + batch-statistics BatchNorm + ReLU [+ skip] in one C call -> (z, stats [3, groups, C], y)."""
    B, D, H, W, cin = a_in.shape
    cout = w.shape[1] if transposed else w.shape[0]
    od, oh, ow = _out_dims(transposed, kd, stride, D, H, W)
    z = torch.empty(B, od, oh, ow, cout, dtype=torch.float32, device=a_in.device)
    y = torch.empty_like(z)
    stats = torch.empty(3, groups, cout, dtype=torch.float32, device=a_in.device)
    lib().mvs_train_block_fwd(ptr(a_in), ptr(w), 1 if transposed else 0, cin, cout, kd, stride[0], stride[1], stride[2], B, D, H, W, ptr(gamma),
                              ptr(beta), float(eps), ptr(running_mean), ptr(running_var), float(momentum), ptr(skip), ptr(ws.zero_bias),
                              ptr(ws.wpack), ptr(ws.sums), ptr(z), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(y), groups, stream_of(a_in))
    return z, stats, y


def train_block_bwd(ws: TrainWorkspace, dy, a_in, z, stats, w, transposed: bool, kd: int, stride, gamma, beta, running_mean, running_var,
                    momentum: float, need_da: bool = True, groups: int = 1):
    """Backward of train_block_fwd in one C call -> (dw, dgamma, dbeta, da or None)."""
    B, D, H, W, cin = a_in.shape
    cout = z.shape[-1]
    dz = torch.empty_like(z)
    dw = torch.empty(w.shape[0], w.shape[1], kd, 3, 3, dtype=torch.float32, device=z.device)
    dgb = torch.empty(2, cout, dtype=torch.float32, device=z.device)
    da = torch.empty_like(a_in) if need_da else None
    lib().mvs_train_block_bwd(ptr(dy), ptr(a_in), ptr(z), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(w), 1 if transposed else 0, cin, cout, kd,
                              stride[0], stride[1], stride[2], B, D, H, W, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var),
                              float(momentum), ptr(ws.zero_bias), ptr(ws.wpack), ptr(ws.sums), ptr(dz), ptr(dw), ptr(dgb[0]), ptr(dgb[1]), ptr(da),
                              groups, stream_of(z))
    return dw, dgb[0], dgb[1], da


def pack_conv_weights_device(w: torch.Tensor, ch: int, tflip: bool = False) -> torch.Tensor:
    """packing.pack_conv_weights_bf16x3 in one launch on the weight's device.  w [Cout, Cin, kd, 3, 3]; tflip: the packed weight is
    W'[co][ci][tap] = w[ci][co][reversed tap] (w then has shape [Cin', Cout'] = [W' columns, W' rows])."""
    w = _f32c(w)
    cout, cin = (w.shape[1], w.shape[0]) if tflip else (w.shape[0], w.shape[1])
    ntap = w.shape[2] * w.shape[3] * w.shape[4]
    n = lib().mvs_pack_conv_weights_elems(cout, cin, ntap, ch)
    if n < 0:
        raise _lib.MvsHipError("pack_conv_weights_device: unsupported shape %s / chunk %d" % (tuple(w.shape), ch))
    out = torch.empty(n, dtype=torch.bfloat16, device=w.device)
    lib().mvs_pack_conv_weights(ptr(w), ptr(out), cout, cin, ntap, ch, 1 if tflip else 0, stream_of(w))
    return out


def pack_deconv_weights_device(w: torch.Tensor, sd: int) -> torch.Tensor:
    """packing.pack_deconv_weights_bf16x3 in one launch.  w [Cin, Cout, 3, 3, 3]."""
    w = _f32c(w)
    cin, cout = w.shape[:2]
    n = lib().mvs_pack_deconv_weights_elems(cin, cout, sd)
    if n < 0:
        raise _lib.MvsHipError("pack_deconv_weights_device: unsupported shape %s" % (tuple(w.shape),))
    out = torch.empty(n, dtype=torch.bfloat16, device=w.device)
    lib().mvs_pack_deconv_weights(ptr(w), ptr(out), cin, cout, sd, stream_of(w))
    return out


def conv3d_wgrad(a_cl: torch.Tensor, g_cl: torch.Tensor, stride: Tuple[int, int, int], kd: int = 3) -> torch.Tensor:
    """Weight gradient of Conv3d(k (kd,3,3), 'same' padding, stride): a_cl [B,D,H,W,CA] input, g_cl [B,OD,OH,OW,CB] output gradient
    -> [CB, CA, kd, 3, 3]."""
    B, D, H, W, CA = a_cl.shape
    CB = g_cl.shape[-1]
    sd, sh, sw = stride
    assert tuple(g_cl.shape[:4]) == (B, (D - 1) // sd + 1, (H - 1) // sh + 1, (W - 1) // sw + 1), "wgrad: gradient shape does not match the stride"
    dw = torch.empty(CB, CA, kd, 3, 3, dtype=torch.float32, device=a_cl.device)
    lib().mvs_conv3d_wgrad(ptr(a_cl), ptr(g_cl), ptr(dw), B, CA, CB, D, H, W, kd, sd, sh, sw, stream_of(a_cl))
    return dw


def conv3d_logits(x_cl: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, precision: int) -> torch.Tensor:
    """CostRegNet's 3x3x3 `prob` head on the MFMA path: x_cl [B,D,H,W,8] -> logits [B,D,H,W]."""
    B, D, H, W, c = x_cl.shape
    assert c == 8
    _act_dtype(x_cl, precision)
    logits = torch.empty(B, D, H, W, dtype=torch.float32, device=x_cl.device)
    lib().mvs_conv3d_logits_fwd(ptr(x_cl), ptr(w_packed), ptr(bias), ptr(logits), B, D, H, W, precision, stream_of(x_cl))
    return logits


def _ptr_array(ts: Sequence[torch.Tensor]):
    return (C.c_void_p * len(ts))(*[ptr(t) for t in ts])


def regnet(kind: int, volume_cl: torch.Tensor, w_packed: Sequence[torch.Tensor], bias: Sequence[torch.Tensor],
           precision: int = 0) -> torch.Tensor:
    """Whole U-Net up to (not including) `prob`: volume_cl [B,D,H,W,8] -> feat_cl [B,D,H,W,8]."""
    B, D, H, W, c = volume_cl.shape
    assert c == 8 and len(w_packed) == 9 and len(bias) == 9
    _act_dtype(volume_cl, precision)
    out = torch.empty_like(volume_cl)
    nbytes = lib().mvs_regnet_workspace_bytes(kind, B, D, H, W)
    ws = _workspace(nbytes, volume_cl.device)
    wa, ba = _ptr_array(w_packed), _ptr_array(bias)
    lib().mvs_regnet_fwd(kind, ptr(volume_cl), C.cast(wa, C.c_void_p), C.cast(ba, C.c_void_p), ptr(out), ptr(ws), nbytes,
                         B, D, H, W, precision, stream_of(volume_cl))
    return out


def regnet_logits(kind: int, volume_cl: torch.Tensor, w_packed: Sequence[torch.Tensor], bias: Sequence[torch.Tensor],
                  prob_w: torch.Tensor, prob_b: torch.Tensor, precision: int) -> torch.Tensor:
    """U-Net + fused 1x1x1 `prob` head: volume_cl [B,D,H,W,8] -> logits [B,D,H,W] (the feature volume stays on chip)."""
    B, D, H, W, c = volume_cl.shape
    assert c == 8 and len(w_packed) == 9 and len(bias) == 9
    _act_dtype(volume_cl, precision)
    logits = torch.empty(B, D, H, W, dtype=torch.float32, device=volume_cl.device)
    nbytes = lib().mvs_regnet_workspace_bytes(kind, B, D, H, W)
    ws = _workspace(nbytes, volume_cl.device)
    wa, ba = _ptr_array(w_packed), _ptr_array(bias)
    lib().mvs_regnet_logits_fwd(kind, ptr(volume_cl), C.cast(wa, C.c_void_p), C.cast(ba, C.c_void_p), ptr(prob_w), ptr(prob_b),
                                ptr(logits), ptr(ws), nbytes, B, D, H, W, precision, stream_of(volume_cl))
    return logits


# ---- a10/a11 ------------------------------------------------------------------------------------
def prob_regress(feat_cl: torch.Tensor, prob_w: torch.Tensor, prob_b: Optional[torch.Tensor], ksize: int, hyp: torch.Tensor,
                 tmp: float, mode: int, conf_n: int = 0, want_volumes: bool = True):
    B, D, H, W, _ = feat_cl.shape
    dev = feat_cl.device
    depth = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    conf = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    need_pre = want_volumes or D not in (4, 8, 16, 32, 48)
    pv = torch.empty(B, D, H, W, dtype=torch.float32, device=dev) if want_volumes else None
    pre = torch.empty(B, D, H, W, dtype=torch.float32, device=dev) if need_pre else None
    lib().mvs_prob_regress_fwd(ptr(feat_cl), ptr(prob_w), ptr(prob_b), ksize, ptr(hyp), float(tmp), mode, conf_n,
                               ptr(depth), ptr(conf), ptr(pv), ptr(pre), B, D, H, W, stream_of(feat_cl))
    return depth, conf, pv, pre


def softmax_regress(logits: torch.Tensor, hyp: torch.Tensor, tmp: float, mode: int, conf_n: int = 0, want_prob: bool = True,
                    conf_prev: Optional[Sequence[torch.Tensor]] = None):
    """-> (depth, conf, prob_volume or None).  conf_prev (round 5): the EARLIER cascade stages' confidence maps (power-of-two smaller);
    the head then also writes the cascade's averaged confidence (DINOv2_mvsformer_model.py:167-177, confidence_average fused into the
    last stage's head) and returns it as a fourth value."""
    lg, hp = _f32c(logits), _f32c(hyp)
    B, D, H, W = lg.shape
    depth = torch.empty(B, H, W, dtype=torch.float32, device=lg.device)
    conf = torch.empty(B, H, W, dtype=torch.float32, device=lg.device)
    pv = torch.empty_like(lg) if want_prob else None
    if conf_prev is None:
        lib().mvs_softmax_regress_fwd(ptr(lg), ptr(hp), float(tmp), mode, conf_n, ptr(depth), ptr(conf), ptr(pv), B, D, H, W, stream_of(lg))
        return depth, conf, pv
    prev = [_f32c(c) for c in conf_prev]
    shifts = []
    for c in prev:
        s = (H // c.shape[1]).bit_length() - 1
        assert c.shape[0] == B and c.shape[1] << s == H and c.shape[2] << s == W, "confidence maps must be power-of-two downsamplings"
        shifts.append(s)
    avg = torch.empty(B, H, W, dtype=torch.float32, device=lg.device)
    pa = _ptr_array(prev) if prev else None
    sa = (C.c_int * max(len(shifts), 1))(*shifts)
    lib().mvs_softmax_regress_confavg_fwd(ptr(lg), ptr(hp), float(tmp), mode, conf_n, ptr(depth), ptr(conf), ptr(pv),
                                          C.cast(pa, C.c_void_p) if prev else None, C.cast(sa, C.c_void_p), len(prev), ptr(avg), B, D, H, W,
                                          stream_of(lg))
    return depth, conf, pv, avg


def softmax_regress_schedule(logits: torch.Tensor, hyp: torch.Tensor, tmp: float, mode: int, conf_n: int, want_prob: bool, next_D: int, ratio: float):
    """Round 5: softmax_regress + schedule_inverse_range(shift=False) of the NEXT stage in one launch
    -> (depth, conf, prob_volume or None, next_hyp [B,next_D,2H,2W])."""
    lg, hp = _f32c(logits), _f32c(hyp)
    B, D, H, W = lg.shape
    depth = torch.empty(B, H, W, dtype=torch.float32, device=lg.device)
    conf = torch.empty(B, H, W, dtype=torch.float32, device=lg.device)
    pv = torch.empty_like(lg) if want_prob else None
    nxt = torch.empty(B, next_D, 2 * H, 2 * W, dtype=torch.float32, device=lg.device)
    lib().mvs_softmax_regress_schedule_fwd(ptr(lg), ptr(hp), float(tmp), mode, conf_n, ptr(depth), ptr(conf), ptr(pv), float(ratio), ptr(nxt), next_D,
                                           B, D, H, W, stream_of(lg))
    return depth, conf, pv, nxt


# ---- section 8f #1: stage-1 transformer regulariser ----------------------------------------------
def position3d(K: torch.Tensor, hyp: torch.Tensor, depth_values: torch.Tensor, pe_range: Optional[torch.Tensor] = None):
    """get_position_3d(normalize=True): K [B,3,3], hyp [B,D,H,W], depth_values [B,n] -> (position3d [B,3,D,H,W],
    range [6] = height_min, height_max, width_min, width_max, depth_min, depth_max).  ``pe_range`` = a previous
    call's range tensor to reuse its first four entries (later cascade stages)."""
    Kc, hp, dv = _f32c(K), _f32c(hyp), _f32c(depth_values)
    B, D, H, W = hp.shape
    compute = pe_range is None
    rng = torch.empty(6, dtype=torch.float32, device=hp.device) if compute else pe_range.clone()
    wsb = lib().mvs_position3d_workspace_bytes()
    ws = _workspace(wsb, hp.device)
    pos = torch.empty(B, 3, D, H, W, dtype=torch.float32, device=hp.device)
    lib().mvs_position3d_fwd(ptr(Kc), ptr(hp), ptr(dv), dv.numel(), ptr(rng), 1 if compute else 0, ptr(ws), wsb, ptr(pos), B, D, H, W, stream_of(hp))
    return pos, rng


def position3d_raw(K: torch.Tensor, hyp: torch.Tensor) -> torch.Tensor:
    """get_position_3d(normalize=False): K [B,3,3], hyp [B,D,H,W] -> the frustum points [B,3,D,H,W] = K^-1 [x, y, 1] * depth."""
    Kc, hp = _f32c(K), _f32c(hyp)
    B, D, H, W = hp.shape
    pos = torch.empty(B, 3, D, H, W, dtype=torch.float32, device=hp.device)
    lib().mvs_position3d_raw_fwd(ptr(Kc), ptr(hp), ptr(pos), B, D, H, W, stream_of(hp))
    return pos


def position_encoding3d(position3d: torch.Tensor, Cc: int, rescale: float = 4.0) -> torch.Tensor:
    """PositionEncoding3D as a tensor: position3d [B,3,D,H,W] -> [B,3C,D,H,W] (position_encoding.py:164-189)."""
    pos = _f32c(position3d)
    B, three, D, H, W = pos.shape
    if three != 3:
        raise _lib.MvsHipError("position3d must be [B,3,D,H,W], got %s" % (tuple(pos.shape),))
    import math
    if Cc < 2 or Cc % 2:
        raise _lib.MvsHipError("PositionEncoding3D needs an even channel count, got %d" % Cc)
    # the frequency table exactly as the reference builds it (fp32 exp of fp32 products, position_encoding.py:169)
    div = torch.exp(torch.arange(0, Cc, 2).float() * (-math.log(10000.0) / Cc)).to(pos.device)
    pe = torch.empty(B, 3 * Cc, D, H, W, dtype=torch.float32, device=pos.device)
    lib().mvs_position_encoding3d_fwd(ptr(pos), ptr(div), ptr(pe), B, Cc, float(rescale), D * H * W, stream_of(pos))
    return pe


def tr_embed(volume_cl: torch.Tensor, pos: Optional[torch.Tensor], pe_w, pe_div, w_packed, bias, ln_w, ln_b, rate, precision: int):
    B, D, H, W, Cc = volume_cl.shape
    assert Cc == 8
    rd, rh, rw = rate
    n = (D // rd) * (H // rh) * (W // rw)
    tokens = torch.empty(B, n, 64, dtype=torch.float32, device=volume_cl.device)
    div = (C.c_float * 4)(*[float(v) for v in pe_div]) if pos is not None else None
    lib().mvs_tr_embed_fwd(ptr(volume_cl), ptr(_f32c(pos)) if pos is not None else None, ptr(pe_w) if pos is not None else None,
                           C.cast(div, C.c_void_p) if div is not None else None, ptr(w_packed), ptr(bias), ptr(ln_w), ptr(ln_b),
                           ptr(tokens), B, D, H, W, rd, rh, rw, precision, stream_of(volume_cl))
    return tokens


def tr_linear(x: torch.Tensor, w_packed, bias, epilogue: int, N: int, precision: int, residual=None, gamma=None, ln_w=None, ln_b=None,
              ln_eps: float = 1e-5):
    B, n, K = x.shape
    y = torch.empty(B, n, N, dtype=torch.float32, device=x.device)
    lib().mvs_tr_linear_fwd(ptr(x), ptr(w_packed), ptr(bias), epilogue, ptr(residual), ptr(gamma), ptr(ln_w), ptr(ln_b),
                            float(ln_eps), ptr(y), B, n, K, N, precision, stream_of(x))
    return y


def tr_attention(x: torch.Tensor, wqkv_packed, heads: int, softmax_scale: float, precision: int, attn_precision: Optional[int] = None) -> torch.Tensor:
    """x [B,n,64] -> softmax(q k^T * scale) v for all heads, [B,n,64] (qkv projection + flash attention, two launches).
    ``attn_precision`` (default = precision): PREC_ATTN16 = one fp16 term per operand like the reference's flash-attn (the module's
    default), PREC_BF16X3 = fp32-equivalent split-bf16 products, PREC_BF16P = the latter with bf16 probabilities in p.v."""
    B, n, Cc = x.shape
    ap = precision if attn_precision is None else attn_precision
    nb = lib().mvs_tr_attention_operand_bytes(B, n, heads)
    buf = torch.empty(3, nb // 2, dtype=torch.bfloat16, device=x.device)
    lib().mvs_tr_qkv_fwd(ptr(x), ptr(wqkv_packed), ptr(buf[0]), ptr(buf[1]), ptr(buf[2]), float(softmax_scale), B, n, heads,
                         precision, ap, stream_of(x))
    out = torch.empty(B, n, Cc, dtype=torch.float32, device=x.device)
    lib().mvs_tr_attention_fwd(ptr(buf[0]), ptr(buf[1]), ptr(buf[2]), ptr(out), B, n, heads, ap, stream_of(x))
    return out


def tr_attention_bwd(qkv: torch.Tensor, o: torch.Tensor, d_o: torch.Tensor, heads: int, softmax_scale: float) -> torch.Tensor:
    """Backward of softmax(scale q k^T) v: qkv [B,n,3*heads*16] (the projection's plain output), o / d_o [B,n,heads*16] -> d_qkv like qkv."""
    B, n, _ = qkv.shape
    qkv, o, d_o = _f32c(qkv), _f32c(o), _f32c(d_o)
    d_qkv = torch.empty_like(qkv)
    ws = torch.empty(2, B * heads * n, dtype=torch.float32, device=qkv.device)
    lib().mvs_tr_attention_bwd(ptr(qkv), ptr(o), ptr(d_o), ptr(d_qkv), ptr(ws[0]), ptr(ws[1]), B, n, heads, float(softmax_scale), stream_of(qkv))
    return d_qkv


def tr_up_prob(tokens: torch.Tensor, w_packed, up_bias, ln_w, ln_b, prob_w, prob_b, dhw, rate, precision: int) -> torch.Tensor:
    B = tokens.shape[0]
    D, H, W = dhw
    logits = torch.empty(B, D, H, W, dtype=torch.float32, device=tokens.device)
    lib().mvs_tr_up_prob_fwd(ptr(tokens), ptr(w_packed), ptr(up_bias), ptr(ln_w), ptr(ln_b), ptr(prob_w), ptr(prob_b), ptr(logits),
                             B, D, H, W, rate[0], rate[1], rate[2], precision, stream_of(tokens))
    return logits


# ---- section 8f #3: depth-map filtering ------------------------------------------------------------
def fusion_pack_cams(cams: torch.Tensor) -> torch.Tensor:
    """cams [..., 2, 4, 4] -> packed {K, K^-1, E, E^-1} [N, campack] for the fusion kernel."""
    c = _f32c(cams).reshape(-1, 2, 4, 4)
    nf = lib().mvs_fusion_campack_floats()
    out = torch.empty(c.shape[0], nf, dtype=torch.float32, device=c.device)
    lib().mvs_fusion_prepare_cams(ptr(c), c.shape[0], ptr(out), stream_of(c))
    return out


def fusion_filter(dynamic: bool, ref_depth, srcs_depth, ref_cam, srcs_cam, *, ref_conf=None, srcs_conf=None, xyd_in=None, in_range_in=None,
                  conf_thresh: float = 0.0, p0: float = 1.0, p1: float = 0.01, vthresh: float = 0.0, want_xyd: bool = False,
                  want_filter: bool = True, want_masks: bool = False, want_points: bool = True):
    """ref_depth [n,h,w]; srcs_depth [n,v,h,w] (or None with xyd_in [n,v,3,h,w]); cameras [n,2,4,4] / [n,v,2,4,4]."""
    n, h, w = ref_depth.shape
    dev = ref_depth.device
    if xyd_in is not None:
        xyd_in = _f32c(xyd_in)
        v = xyd_in.shape[1]
    else:
        v = srcs_depth.shape[1]
    rc = fusion_pack_cams(ref_cam) if ref_cam is not None else None
    sc = fusion_pack_cams(srcs_cam) if srcs_cam is not None else None
    out = {}
    if want_xyd:
        out["reproj_xyd"] = torch.empty(n, v, 3, h, w, dtype=torch.float32, device=dev)
        if not dynamic:
            out["in_range"] = torch.empty(n, v, h, w, dtype=torch.float32, device=dev)
    if want_filter:
        out["depth"] = torch.empty(n, h, w, dtype=torch.float32, device=dev)
        out["geo_mask"] = torch.empty(n, h, w, dtype=torch.uint8, device=dev)
        out["mask"] = torch.empty(n, h, w, dtype=torch.uint8, device=dev)
        if want_masks:
            out["vis_masks"] = torch.empty((n, v, v - 1, h, w) if dynamic else (n, v, h, w), dtype=torch.uint8, device=dev)
        if want_points and rc is not None:
            out["points"] = torch.empty(n, 3, h, w, dtype=torch.float32, device=dev)
    g = out.get
    lib().mvs_fusion_filter_fwd(1 if dynamic else 0, ptr(ref_depth), ptr(ref_conf), ptr(srcs_depth), ptr(srcs_conf), ptr(rc), ptr(sc),
                                ptr(xyd_in), ptr(in_range_in), float(conf_thresh), float(p0), float(p1), float(vthresh),
                                ptr(g("reproj_xyd")), ptr(g("in_range")), ptr(g("vis_masks")), ptr(g("depth")), ptr(g("geo_mask")),
                                ptr(g("mask")), ptr(g("points")), n, v, h, w, stream_of(ref_depth))
    return out


def fusion_ave(ref_depth, reproj_xyd, masks):
    n, h, w = ref_depth.shape
    x = _f32c(reproj_xyd)
    out = torch.empty(n, h, w, dtype=torch.float32, device=ref_depth.device)
    lib().mvs_fusion_ave_fwd(ptr(ref_depth), ptr(x), ptr(masks), ptr(out), n, x.shape[1], h, w, stream_of(ref_depth))
    return out


PLY_RECORD_BYTES = 15


def pointcloud_append(mask, points, rgb, records, counter, view_counts=None, view_slot: int = 0):
    """Append one view's kept pixels as packed PLY vertex records: mask [h,w] (bool / uint8), points [3,h,w] fp32, rgb [h,w,3]
    uint8 -> records (uint8, capacity * 15 bytes) from record counter[0] (int32 [1], advanced); view_counts (int32) [view_slot] =
    the view's count.  Stream-ordered, no synchronisation; the caller keeps counter + h*w <= capacity."""
    h, w = mask.shape[-2:]
    m = mask.reshape(h, w).contiguous()
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    pts, col = _f32c(points).reshape(3, h, w), rgb.reshape(h, w, 3).contiguous()
    assert m.dtype == torch.uint8 and col.dtype == torch.uint8 and records.dtype == torch.uint8 and counter.dtype == torch.int32
    nbytes = lib().mvs_pointcloud_workspace_bytes(h, w)
    ws = _workspace(nbytes, m.device)
    lib().mvs_pointcloud_append(ptr(m), ptr(pts), ptr(col), h, w, ptr(ws), nbytes, ptr(counter), ptr(view_counts), int(view_slot),
                                ptr(records), records.numel() // PLY_RECORD_BYTES, stream_of(m))


# ---- gipuma route (misc/gipuma.py) -------------------------------------------
def gipuma_prepare_cams(cams) -> Tuple[torch.Tensor, torch.Tensor]:
    """cams [N,2,4,4] (host or device; float32 values) -> (view_consts [N, view_floats], pair_consts [N, N, pair_floats]), fp32
    host tensors prepared in fp64 on the host.  Raises on a singular P[:, :3]."""
    import numpy as np
    c = np.ascontiguousarray(torch.as_tensor(cams).detach().cpu().numpy(), dtype=np.float32).reshape(-1, 2, 4, 4)
    n = c.shape[0]
    vf, pf = lib().mvs_gipuma_view_floats(), lib().mvs_gipuma_pair_floats()
    views = np.zeros((n, vf), np.float32)
    pairs = np.zeros((n, n, pf), np.float32)
    lib().mvs_gipuma_prepare_cams(c.ctypes.data, n, views.ctypes.data, pairs.ctypes.data)
    return torch.from_numpy(views), torch.from_numpy(pairs)


def gipuma_prepare_view(depth, keep, rgb, depth_out, color_out) -> None:
    """One view's device slot: depth_out [h,w] fp32 = keep ? depth : 0 (keep [h,w] bool / uint8, None = keep all), color_out
    [h,w] int32 = packed rgb [h,w,3] uint8.  Stream-ordered."""
    h, w = depth.shape[-2:]
    d = _f32c(depth).reshape(h, w)
    k = None if keep is None else keep.reshape(h, w).contiguous()
    if k is not None and k.dtype == torch.bool:
        k = k.view(torch.uint8)
    col = rgb.reshape(h, w, 3).contiguous()
    assert col.dtype == torch.uint8 and depth_out.dtype == torch.float32 and color_out.dtype == torch.int32
    assert depth_out.is_contiguous() and color_out.is_contiguous() and depth_out.numel() == h * w == color_out.numel()
    lib().mvs_gipuma_prepare_view(ptr(d), ptr(k), ptr(col), h, w, ptr(depth_out), ptr(color_out), stream_of(d))


def gipuma_fuse_view(depths, colors, used, view_consts, pair_consts, r: int, *, depth_min: float, depth_max: float, disp_thresh: float,
                     num_consistent: float, mask, points, rgb, skipped=None) -> None:
    """Fusion launch of reference view r: depths [N,h,w] fp32, colors [N,h,w] int32, used [N,h,w] uint8 (read at r, marked
    elsewhere), constants from gipuma_prepare_cams on the same device -> mask [h,w] uint8, points [3,h,w] fp32, rgb [h,w,3] uint8
    (kept pixels only), skipped [h,w] uint8 (optional).  Stream-ordered, no synchronisation."""
    n, h, w = depths.shape
    for t, dt in ((depths, torch.float32), (colors, torch.int32), (used, torch.uint8), (view_consts, torch.float32),
                  (pair_consts, torch.float32), (mask, torch.uint8), (points, torch.float32), (rgb, torch.uint8)):
        assert t.dtype == dt and t.is_contiguous(), "gipuma_fuse_view: bad tensor"
    assert colors.shape == used.shape == depths.shape and mask.numel() == h * w and points.numel() == 3 * h * w and rgb.numel() == 3 * h * w
    assert view_consts.shape[0] == n and pair_consts.shape[:2] == (n, n)
    if skipped is not None:
        assert skipped.dtype == torch.uint8 and skipped.is_contiguous() and skipped.numel() == h * w
    lib().mvs_gipuma_fuse_view(ptr(depths), ptr(colors), ptr(used), ptr(view_consts), ptr(pair_consts), n, h, w, int(r),
                               float(depth_min), float(depth_max), float(disp_thresh), float(num_consistent), ptr(mask), ptr(points),
                               ptr(rgb), ptr(skipped), stream_of(depths))


# ---- colmap2mvsnet (colmap2mvsnet.py) ----------------------------------------
COLMAP_MAX_IMAGES = 16384


def _i32c(t: torch.Tensor) -> torch.Tensor:
    assert t.dtype == torch.int32, "expected int32, got %s" % t.dtype
    return t.contiguous()


def _f64c(t: torch.Tensor) -> torch.Tensor:
    assert t.dtype == torch.float64, "expected float64, got %s" % t.dtype
    return t.contiguous()


def colmap_depths(obs_img, obs_pt, xyz, erow) -> torch.Tensor:
    """z [n] fp64 of n observations: obs_img / obs_pt int32 [n] (image, dense point index), xyz fp64 [P,3], erow fp64 [N,4] (row 2 of
    each image's extrinsic).  Stream-ordered."""
    oi, op, x, e = _i32c(obs_img), _i32c(obs_pt), _f64c(xyz), _f64c(erow)
    z = torch.empty(oi.numel(), dtype=torch.float64, device=oi.device)
    lib().mvs_colmap_depths(ptr(oi), ptr(op), oi.numel(), ptr(x), ptr(e), ptr(z), stream_of(oi))
    return z


def colmap_scores(img_ptr, img_pts, img_mult, pt_ptr, pt_imgs, xyz, centres, *, theta0: float, den1: float, den2: float,
                  max_pairs: int) -> torch.Tensor:
    """score [N,N] fp64 of the view selection: the per-image CSR (img_ptr int32 [N+1], img_pts / img_mult int32: sorted unique dense
    point indices and their multiplicity), the per-point CSR of ascending images (pt_ptr int32 [P+1], pt_imgs int32), xyz fp64 [P,3],
    centres fp64 [N,3]; den = 2 sigma^2; max_pairs >= the number of co-visible pairs.  Stream-ordered, no synchronisation."""
    ip, ipt, im, pp, pim = (_i32c(t) for t in (img_ptr, img_pts, img_mult, pt_ptr, pt_imgs))
    x, c = _f64c(xyz), _f64c(centres)
    n, p = ip.numel() - 1, pp.numel() - 1
    dev = ip.device
    nbytes = lib().mvs_colmap_workspace_bytes(n)
    if nbytes == 0:
        raise ValueError("colmap_scores: %d images (1..%d)" % (n, COLMAP_MAX_IMAGES))
    ws = _workspace(nbytes, dev)
    flags = torch.empty(n * n, dtype=torch.uint8, device=dev)
    pairs = torch.empty(max(int(max_pairs), 1), dtype=torch.int32, device=dev)
    score = torch.empty(n, n, dtype=torch.float64, device=dev)
    lib().mvs_colmap_scores(ptr(ip), ptr(ipt), ptr(im), n, ptr(pp), ptr(pim), p, ptr(x), ptr(c), float(theta0), float(den1),
                            float(den2), int(max_pairs), ptr(flags), ptr(pairs), ptr(ws), nbytes, ptr(score), stream_of(ip))
    return score


# ---- a13-a16 ------------------------------------------------------------------------------------
def depth_regression(p: torch.Tensor, depth_values: torch.Tensor) -> torch.Tensor:
    pp, dv = _f32c(p), _f32c(depth_values)
    B, D, H, W = pp.shape
    out = torch.empty(B, H, W, dtype=torch.float32, device=pp.device)
    lib().mvs_depth_regression_fwd(ptr(pp), ptr(dv), ptr(out), B, D, H, W, stream_of(pp))
    return out


def conf_regression(p: torch.Tensor, n: int) -> torch.Tensor:
    pp = _f32c(p)
    B, D, H, W = pp.shape
    out = torch.empty(B, H, W, dtype=torch.float32, device=pp.device)
    lib().mvs_conf_regression_fwd(ptr(pp), int(n), ptr(out), B, D, H, W, stream_of(pp))
    return out


def init_range(depth_values: torch.Tensor, ndepths: int, H: int, W: int, inverse: bool) -> torch.Tensor:
    """depth_values [B,N] (one range per image) or [B,H,W,N] (one per pixel, module.py:683-688 / 698-703) -> hypotheses [B,D,H,W]."""
    dv = _f32c(depth_values)
    if dv.dim() == 4:
        B, h, w, N = dv.shape
        if (h, w) != (H, W):
            raise _lib.MvsHipError("per-pixel initial ranges %s do not match the %dx%d hypothesis maps" % (tuple(dv.shape), H, W))
        hyp = torch.empty(B, ndepths, H, W, dtype=torch.float32, device=dv.device)
        lib().mvs_init_range_pixel_fwd(ptr(dv), N, 1 if inverse else 0, ptr(hyp), B, ndepths, H, W, stream_of(dv))
        return hyp
    B, N = dv.shape
    hyp = torch.empty(B, ndepths, H, W, dtype=torch.float32, device=dv.device)
    lib().mvs_init_range_fwd(ptr(dv), N, 1 if inverse else 0, ptr(hyp), B, ndepths, H, W, stream_of(dv))
    return hyp


def schedule_inverse_range(prev_depth: torch.Tensor, prev_hyp: torch.Tensor, ndepths: int, ratio: float, H: int, W: int,
                           shift: bool = False) -> torch.Tensor:
    d, h = _f32c(prev_depth), _f32c(prev_hyp)
    B, Dp = h.shape[:2]
    assert tuple(d.shape[-2:]) == (H // 2, W // 2) and tuple(h.shape[-2:]) == (H // 2, W // 2)
    hyp = torch.empty(B, ndepths, H, W, dtype=torch.float32, device=d.device)
    lib().mvs_schedule_inverse_range_fwd(ptr(d), ptr(h), Dp, float(ratio), 1 if shift else 0, ptr(hyp), B, ndepths, H, W, stream_of(d))
    return hyp


def schedule_range(prev_depth: torch.Tensor, ndepths: int, interval: torch.Tensor, H: int, W: int) -> torch.Tensor:
    d = _f32c(prev_depth)
    B = d.shape[0]
    per_pixel = interval.dim() == 3                       # [B,H/2,W/2] intervals (module.py:731-732 takes them as they are)
    if per_pixel:
        if tuple(interval.shape) != tuple(d.shape):
            raise _lib.MvsHipError("per-pixel depth intervals %s do not match the depth map %s" % (tuple(interval.shape), tuple(d.shape)))
        itv = _f32c(interval)
    else:
        itv = _f32c(interval.reshape(-1).expand(B) if interval.numel() == 1 else interval.reshape(B))
    hyp = torch.empty(B, ndepths, H, W, dtype=torch.float32, device=d.device)
    lib().mvs_schedule_range_fwd(ptr(d), ptr(itv), 1 if per_pixel else 0, ptr(hyp), B, ndepths, H, W, stream_of(d))
    return hyp


def confidence_average(confs: Sequence[torch.Tensor], H: int, W: int) -> torch.Tensor:
    confs = [_f32c(c) for c in confs]
    B = confs[0].shape[0]
    shifts = []
    for c in confs:
        s = (H // c.shape[1]).bit_length() - 1
        assert c.shape[1] << s == H and c.shape[2] << s == W, "confidence maps must be power-of-two downsamplings"
        shifts.append(s)
    out = torch.empty(B, H, W, dtype=torch.float32, device=confs[0].device)
    pa = _ptr_array(confs)
    sa = (C.c_int * len(shifts))(*shifts)
    lib().mvs_confidence_average(C.cast(pa, C.c_void_p), C.cast(sa, C.c_void_p), len(confs), ptr(out), B, H, W, stream_of(out))
    return out


def ncdhw_to_cl(x: torch.Tensor) -> torch.Tensor:
    x = _f32c(x)
    B, Cc, D, H, W = x.shape
    y = torch.empty(B, D, H, W, Cc, dtype=torch.float32, device=x.device)
    lib().mvs_ncdhw_to_cl(ptr(x), ptr(y), B, Cc, D, H, W, stream_of(x))
    return y


def cl_to_ncdhw(x_cl: torch.Tensor) -> torch.Tensor:
    B, D, H, W, Cc = x_cl.shape
    y = torch.empty(B, Cc, D, H, W, dtype=torch.float32, device=x_cl.device)
    lib().mvs_cl_to_ncdhw(ptr(x_cl), ptr(y), B, Cc, D, H, W, stream_of(x_cl))
    return y


def _resize_source(t: torch.Tensor, what: str) -> None:
    if not torch.is_tensor(t) or t.dim() != 4 or t.dtype != torch.float32 or min(t.shape) < 1 or min(t.stride()) < 0:
        raise ValueError("%s must be a fp32 tensor [N, C, H, W] with no empty axis; got %s"
                         % (what, (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t)))


def resize_bicubic(img: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """F.interpolate(img, (h, w), mode="bicubic", align_corners=False) without antialiasing (DINOv2_mvsformer_model.py:76): img fp32
    [N, C, H, W] with ANY strides (read in place: a [B V, 3, H, W] view of [B, V, 3, H, W] is not copied) -> contiguous fp32 [N, C, h, w].
    Any scale (taps skip pixels when scaling down by more than 2), any axis length >= 1."""
    _resize_source(img, "img")
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError("resize_bicubic: the output size must be at least 1 x 1; got %d x %d" % (h, w))
    N, Cc, H, W = img.shape
    out = torch.empty(N, Cc, h, w, dtype=torch.float32, device=img.device)
    lib().mvs_resize_bicubic_fwd(_base_ptr(img), img.stride(0), img.stride(1), img.stride(2), img.stride(3), ptr(out), N, Cc, H, W, h, w,
                                 stream_of(img))
    return out


def resize_bilinear_add(base: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """base + F.interpolate(x, base.shape[-2:], mode="bilinear", align_corners=False) (DINOv2_mvsformer_model.py:80-88): base fp32
    [N, C, h, w], x fp32 [N, C, h', w'] (any strides) -> a fresh contiguous fp32 [N, C, h, w].  (h', w') == (h, w): base + x bit for bit."""
    _resize_source(base, "base")
    _resize_source(x, "x")
    if x.shape[:2] != base.shape[:2] or x.device != base.device:
        raise ValueError("resize_bilinear_add: base %s on %s and x %s on %s must agree in N, C and device"
                         % (tuple(base.shape), base.device, tuple(x.shape), x.device))
    base = base.contiguous()
    N, Cc, h, w = base.shape
    out = torch.empty_like(base)
    lib().mvs_resize_bilinear_add_fwd(ptr(base), _base_ptr(x), x.stride(0), x.stride(1), x.stride(2), x.stride(3), ptr(out), N, Cc, h, w,
                                      x.shape[2], x.shape[3], stream_of(base))
    return out


# ---- a scene's depth inference: image preparation and output packing (csrc/scene_kernels.hip) ----
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def normalise_table(mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD) -> torch.Tensor:
    """fp32 [3, 256] on the host: ToTensor + Normalize of every byte value, ``((u / 255) - mean[c]) / std[c]`` as torch evaluates it
    (general_eval.py:29-32), so a lookup is bit-equal to the transform."""
    u = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    return u[None].sub(m[:, None]).div(s[:, None]).contiguous()


def image_prepare(src: torch.Tensor, H: int, W: int, table: torch.Tensor, pad_rows: int = 0, planar: Optional[torch.Tensor] = None,
                  resized: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """A decoded image, uint8 RGB [h, w, 3], -> (fp32 planar [3, H, W] normalised through ``table``, uint8 [H, W, 3]): ``pad_rows``
    replicated rows above and below (the "tt" pad of general_eval.py:115-116), the 8-bit linear resize to H x W (OpenCV's fixed-point
    arithmetic; equal sizes: the identity), ToTensor and Normalize in one pass.  ``planar`` / ``resized``: contiguous tensors of those shapes
    to write into (a slot of a view cache); fresh ones otherwise."""
    if not torch.is_tensor(src) or src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3 or min(src.shape) < 1:
        raise ValueError("image_prepare: src must be a uint8 tensor [h, w, 3] with no empty axis; got %s"
                         % ((src.dtype, tuple(src.shape)) if torch.is_tensor(src) else type(src),))
    H, W, pad_rows = int(H), int(W), int(pad_rows)
    if H < 1 or W < 1:
        raise ValueError("image_prepare: the output size must be at least 1 x 1; got %d x %d" % (H, W))
    if not torch.is_tensor(table) or table.dtype != torch.float32 or tuple(table.shape) != (3, 256) or table.device != src.device:
        raise ValueError("image_prepare: table must be a fp32 tensor [3, 256] on the image's device (ops.normalise_table())")
    src, table = src.contiguous(), table.contiguous()
    if planar is None:
        planar = torch.empty(3, H, W, dtype=torch.float32, device=src.device)
    if resized is None:
        resized = torch.empty(H, W, 3, dtype=torch.uint8, device=src.device)
    for t, dt, shape, what in ((planar, torch.float32, (3, H, W), "planar"), (resized, torch.uint8, (H, W, 3), "resized")):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != src.device:
            raise ValueError("image_prepare: %s must be a contiguous %s tensor %s on the image's device" % (what, dt, list(shape)))
    lib().mvs_image_prepare_fwd(ptr(src), src.shape[0], src.shape[1], pad_rows, ptr(table), ptr(planar), ptr(resized), H, W, stream_of(src))
    return planar, resized


def depth_outputs_pack(depth: torch.Tensor, conf: torch.Tensor, reg_conf: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """depth, conf (and stage 4's confidence for --combine_reg_conf) fp32 [H, W] -> uint8 [5 H W]: the depth rows bottom-up as fp32 bytes
    (the body ``save_pfm`` writes after its flipud), then ``uint8(c * 255)`` with c = conf or (conf * 3 + reg_conf) / 4 (test.py:280-285)."""
    maps = [("depth", depth), ("conf", conf)] + ([("reg_conf", reg_conf)] if reg_conf is not None else [])
    for what, t in maps:
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or min(t.shape) < 1 or t.shape != depth.shape or t.device != depth.device:
            raise ValueError("depth_outputs_pack: %s must be a fp32 tensor [H, W] with no empty axis, all maps of one size on one device; got %s"
                             % (what, (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t)))
    H, W = depth.shape
    if out is None:
        out = torch.empty(5 * H * W, dtype=torch.uint8, device=depth.device)
    elif out.dtype != torch.uint8 or out.numel() != 5 * H * W or not out.is_contiguous() or out.device != depth.device:
        raise ValueError("depth_outputs_pack: out must be a contiguous uint8 tensor of 5 H W = %d bytes on the maps' device" % (5 * H * W))
    lib().mvs_depth_outputs_pack_fwd(ptr(depth.contiguous()), ptr(conf.contiguous()), ptr(None if reg_conf is None else reg_conf.contiguous()),
                                     ptr(out), H, W, stream_of(depth))
    return out


# ---- the multi-stage depth losses and the validation metrics (csrc/loss_kernels.hip) ----
METRICS_MAX_T = 8


def _loss_map(t, what: str, fn: str, shape=None) -> torch.Tensor:
    """A fp32 map [B, H, W] with no empty axis (of `shape` when given) -> contiguous."""
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 3 or min(t.shape) < 1 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError("%s: %s must be a fp32 tensor %s with no empty axis; got %s"
                         % (fn, what, "[B, H, W]" if shape is None else list(shape), (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t)))
    return t.contiguous()


def _loss_volume(t, what: str, fn: str, bhw=None) -> torch.Tensor:
    """A fp32 volume [B, D, H, W] with D >= 2 (over the maps `bhw` when given) -> contiguous."""
    ok = torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 4 and min(t.shape) >= 1 and t.shape[1] >= 2
    if ok and bhw is not None:
        ok = (t.shape[0], t.shape[2], t.shape[3]) == tuple(bhw)
    if not ok:
        raise ValueError("%s: %s must be a fp32 tensor [B, D, H, W] with D >= 2 that matches the maps; got %s"
                         % (fn, what, (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t)))
    return t.contiguous()


def _loss_workspace(pixels: int, like: torch.Tensor):
    nbytes = lib().mvs_loss_workspace_bytes(pixels)
    if nbytes == 0:
        raise ValueError("the losses take 1 <= B H W < 2^31 pixels; got %d" % pixels)
    return _workspace(nbytes, like.device), nbytes                                              # sized from the launch grid


def ce_loss_fwd(logits: torch.Tensor, hyp: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, inverse: bool, weight: float = 1.0):
    """The "ce" stage loss (losses.py:31-62): logits, hyp fp32 [B,D,H,W], gt, mask fp32 [B,H,W] -> (loss fp32 [1] = weight * mean over the N
    valid pixels of lse - logit[bin], N int32 [1], index int32 [B,H,W] (the target plane in stored order, -1 = not valid), lse fp32
    [B,H,W]).  Two launches, no synchronisation; N = 0 gives NaN."""
    x = _loss_volume(logits, "logits", "ce_loss_fwd")
    B, D, H, W = x.shape
    h = _loss_volume(hyp, "hyp", "ce_loss_fwd", (B, H, W))
    if h.shape[1] != D:
        raise ValueError("ce_loss_fwd: logits %s and hyp %s differ in D" % (tuple(x.shape), tuple(h.shape)))
    g, m = _loss_map(gt, "gt", "ce_loss_fwd", (B, H, W)), _loss_map(mask, "mask", "ce_loss_fwd", (B, H, W))
    ws, nbytes = _loss_workspace(B * H * W, x)
    index = torch.empty(B, H, W, dtype=torch.int32, device=x.device)
    lse = torch.empty(B, H, W, dtype=torch.float32, device=x.device)
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    count = torch.empty(1, dtype=torch.int32, device=x.device)
    lib().mvs_ce_loss_fwd(ptr(x), ptr(h), ptr(g), ptr(m), 1 if inverse else 0, float(weight), ptr(index), ptr(lse), ptr(ws), nbytes,
                          ptr(loss), ptr(count), B, D, H, W, stream_of(x))
    return loss, count, index, lse


def ce_loss_bwd(logits: torch.Tensor, index: torch.Tensor, lse: torch.Tensor, grad_loss: torch.Tensor, count: torch.Tensor,
                weight: float = 1.0) -> torch.Tensor:
    """grad_logits [B,D,H,W] = (grad_loss * weight / N) * (exp(logit - lse) - [plane == index]) where index >= 0, else 0; grad_loss fp32 [1]
    and N int32 [1] are read on the device.  One launch that writes the whole volume."""
    x = _loss_volume(logits, "logits", "ce_loss_bwd")
    B, D, H, W = x.shape
    if not torch.is_tensor(index) or index.dtype != torch.int32 or tuple(index.shape) != (B, H, W):
        raise ValueError("ce_loss_bwd: index must be an int32 tensor %s" % [B, H, W])
    if not torch.is_tensor(count) or count.dtype != torch.int32 or count.numel() != 1:
        raise ValueError("ce_loss_bwd: count must be an int32 tensor of one element")
    l = _loss_map(lse, "lse", "ce_loss_bwd", (B, H, W))
    g = _f32c(grad_loss).reshape(1)
    grad = torch.empty_like(x)
    lib().mvs_ce_loss_bwd(ptr(x), ptr(index.contiguous()), ptr(l), ptr(g), ptr(count.contiguous()), float(weight), ptr(grad), B, D, H, W,
                          stream_of(x))
    return grad


def _reg_inputs(fn, depth, gt, mask, interval, hyp):
    d = _loss_map(depth, "depth", fn)
    B, H, W = d.shape
    g, m = _loss_map(gt, "gt", fn, (B, H, W)), _loss_map(mask, "mask", fn, (B, H, W))
    if interval is not None:
        if not torch.is_tensor(interval) or interval.dtype != torch.float32 or tuple(interval.shape) != (B,):
            raise ValueError("%s: interval must be a fp32 tensor [%d] (one per image) or None" % (fn, B))
        interval = interval.contiguous()
    if hyp is not None:
        hyp = _loss_volume(hyp, "hyp", fn, (B, H, W))
    return d, g, m, interval, hyp, B, (hyp.shape[1] if hyp is not None else 1), H, W


def reg_loss_fwd(depth: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, interval: Optional[torch.Tensor] = None,
                 hyp: Optional[torch.Tensor] = None, inverse: bool = False, weight: float = 1.0):
    """The "reg" stage loss (losses.py:64-97 without log_var; reg_loss, simple_loss): smooth L1 (beta 1) of depth / interval[b] against
    gt / interval[b] over mask > 0.5 (interval None: 1); hyp [B,D,H,W] given = clip_func "dynamic", every pixel's loss clamped from above by
    the hypotheses' range / interval[b].  -> (loss fp32 [1] = weight * mean, N int32 [1]).  Two launches; N = 0 gives NaN."""
    d, g, m, itv, h, B, D, H, W = _reg_inputs("reg_loss_fwd", depth, gt, mask, interval, hyp)
    ws, nbytes = _loss_workspace(B * H * W, d)
    loss = torch.empty(1, dtype=torch.float32, device=d.device)
    count = torch.empty(1, dtype=torch.int32, device=d.device)
    lib().mvs_reg_loss_fwd(ptr(d), ptr(g), ptr(m), ptr(itv), ptr(h), 1 if inverse else 0, float(weight), ptr(ws), nbytes, ptr(loss),
                           ptr(count), B, D, H, W, stream_of(d))
    return loss, count


def reg_loss_bwd(depth: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, interval: Optional[torch.Tensor], hyp: Optional[torch.Tensor],
                 inverse: bool, grad_loss: torch.Tensor, count: torch.Tensor, weight: float = 1.0) -> torch.Tensor:
    """grad_depth [B,H,W] of reg_loss_fwd (recomputed from the inputs; the clamp passes the gradient where loss <= range); grad_loss fp32 [1]
    and N int32 [1] are read on the device.  One launch that writes the whole map."""
    d, g, m, itv, h, B, D, H, W = _reg_inputs("reg_loss_bwd", depth, gt, mask, interval, hyp)
    if not torch.is_tensor(count) or count.dtype != torch.int32 or count.numel() != 1:
        raise ValueError("reg_loss_bwd: count must be an int32 tensor of one element")
    go = _f32c(grad_loss).reshape(1)
    grad = torch.empty_like(d)
    lib().mvs_reg_loss_bwd(ptr(d), ptr(g), ptr(m), ptr(itv), ptr(h), 1 if inverse else 0, ptr(go), ptr(count.contiguous()), float(weight),
                           ptr(grad), B, D, H, W, stream_of(d))
    return grad


def depth_metrics(depth_est: torch.Tensor, depth_gt: torch.Tensor, mask: torch.Tensor, thres: Sequence[float],
                  bands: Sequence[Optional[Tuple[float, float]]], interval: Optional[torch.Tensor] = None, divisor: float = 1.0,
                  per_sample: bool = False):
    """The counts and sums behind Thres_metrics / AbsDepthError_metrics (utils.py:156-189) for T thresholds and T bands per image, in one
    metrics launch plus its finalize: depth_est, depth_gt fp32 [B,H,W]; mask fp32 (> 0.5) or bool / uint8 (!= 0).  A threshold is
    ``base * factor`` formed on the device in fp64 and rounded to fp32, base = interval[b if per_sample else 0] / divisor (interval None: 1)
    and the factors the Python numbers given here; a band of None is "no band".
    -> (counts int32 [B, 1 + 2 T]: valid, T of err > thres, T of lo <= err <= hi; sums fp64 [B, T] of the errors inside the bands; means
    fp32 [B + 1, 2 T]: per image T ratios and T band means, row B their mean over the images)."""
    e = _loss_map(depth_est, "depth_est", "depth_metrics")
    B, H, W = e.shape
    g = _loss_map(depth_gt, "depth_gt", "depth_metrics", (B, H, W))
    if not torch.is_tensor(mask) or tuple(mask.shape) != (B, H, W) or mask.dtype not in (torch.float32, torch.bool, torch.uint8):
        raise ValueError("depth_metrics: mask must be a fp32, bool or uint8 tensor %s; got %s"
                         % ([B, H, W], (mask.dtype, tuple(mask.shape)) if torch.is_tensor(mask) else type(mask)))
    m = mask.contiguous()
    T = len(thres)
    if not 1 <= T <= METRICS_MAX_T or len(bands) != T:
        raise ValueError("depth_metrics: 1 to %d thresholds and as many bands; got %d and %d" % (METRICS_MAX_T, T, len(bands)))
    if interval is not None:
        if not torch.is_tensor(interval) or interval.dtype != torch.float32 or interval.dim() != 1 or interval.numel() != B:
            raise ValueError("depth_metrics: interval must be a fp32 tensor [%d] or None" % B)
        interval = interval.contiguous()
    nan = float("nan")
    th = (C.c_double * T)(*[float(t) for t in thres])
    lo = (C.c_double * T)(*[nan if b is None else float(b[0]) for b in bands])
    hi = (C.c_double * T)(*[nan if b is None else float(b[1]) for b in bands])
    nbytes = lib().mvs_depth_metrics_workspace_bytes(B, H, W, T)
    if nbytes == 0:
        raise ValueError("depth_metrics: 1 <= B <= 65535 images and B H W < 2^31 pixels; got %s" % ([B, H, W],))
    ws = _workspace(nbytes, e.device)
    counts = torch.empty(B, 1 + 2 * T, dtype=torch.int32, device=e.device)
    sums = torch.empty(B, T, dtype=torch.float64, device=e.device)
    means = torch.empty(B + 1, 2 * T, dtype=torch.float32, device=e.device)
    lib().mvs_depth_metrics(ptr(e), ptr(g), ptr(m), 0 if m.dtype == torch.float32 else 1, ptr(interval), float(divisor),
                            1 if per_sample else 0, C.cast(th, C.c_void_p), C.cast(lo, C.c_void_p), C.cast(hi, C.c_void_p), T, ptr(ws),
                            nbytes, ptr(counts), ptr(sums), ptr(means), B, H, W, stream_of(e))
    return counts, sums, means
