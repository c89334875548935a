"""float64 restatements of the tuned 3-D MFMA convolution family (csrc/conv_kernels.hip, csrc/conv_bf16x3_kernels.hip) for
tests/test_conv3d_family*.py: Conv3d (kd,3,3) + bias + optional ReLU, ConvTranspose3d 3x3x3 (stride (sd,2,2)) + bias + optional ReLU +
optional skip add AFTER the ReLU, the fused 1x1x1 `prob` head over the 8 channels after the skip add, the one-channel 3x3x3 head, the
OPERAND MODEL of every storage format, and per output element the absolute sum S = sum |x| |w| the error bars are stated in.

Everything is plain torch in float64 on channel-last tensors [B, D, H, W, C]; nothing here calls the library.

Operand models (what the float64 reference is evaluated on, so that a format's own input rounding is not charged to the kernel):

    format      activations                      weights
    fp32        x                                w
    bf16x3      x (the kernel splits it)         w
    split       x (the kernel is fed ops.to_split(x), the result read back through ops.from_split)        w
    f16x2       x.half()                         fp16 hi + lo of w, as packing._split_f16 does
    f16         x.half()                         w.half()
"""
import os
import re

import torch
import torch.nn.functional as F

from mvsformerplusplus_amd import _lib, packing

CONV_CFG_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mvsformerplusplus_amd", "csrc", "conv_cfg.h")

FORMATS = ("fp32", "bf16x3", "split", "f16x2", "f16")
CODE = {"fp32": _lib.PREC_FP32, "bf16x3": _lib.PREC_BF16X3, "split": _lib.PREC_BF16X3_SPLIT, "f16x2": _lib.PREC_F16X2, "f16": _lib.PREC_F16}
F16_FORMATS = ("f16x2", "f16")
SPLIT_BF16_FORMATS = ("bf16x3", "split")


# ---------------------------------------------------------------------------------------------------------------- the tile tables
def _table(src, defs, name):
    lines = src[src.index("#define %s(X)" % name):].split("\n")
    body = []
    for ln in lines:                                     # the macro runs as long as its lines end in a backslash
        body.append(ln)
        if not ln.rstrip().endswith("\\"):
            break
    rows = re.findall(r"X\(([^)]*)\)", "\n".join(body[1:]))
    return [tuple(int(defs.get(t.strip(), t.strip())) for t in r.split(",")) for r in rows]


def tile_tables():
    """-> (conv rows (CIN, COUT, KD, SD, SH, SW, TD, TH, CH), deconv rows (CIN, COUT, SD, TDM, THM)) read from csrc/conv_cfg.h with the
    default values of its MVS_* tile macros.  A conv tile is TD x TH x 16 OUTPUT voxels, a deconv tile TDM x THM x 16 INPUT voxels."""
    src = open(CONV_CFG_H).read()
    defs = dict(re.findall(r"^#define\s+(MVS_\w+)\s+(\d+)\s*$", src, re.M))
    return _table(src, defs, "MVS_CONV_TABLE"), _table(src, defs, "MVS_DECONV_TABLE")


def conv_out_dims(D, H, W, kd, stride):
    return (D + 2 * (kd // 2) - kd) // stride[0] + 1, (H - 1) // stride[1] + 1, (W - 1) // stride[2] + 1


def ceil_div(a, b):
    return -(-a // b)


def conv_ntiles(D, H, W, row):
    """Tiles per batch item of a conv row at input size D x H x W (launch_conv_bf)."""
    cin, cout, kd, sd, sh, sw, TD, TH, ch = row
    od, oh, ow = conv_out_dims(D, H, W, kd, (sd, sh, sw))
    return ceil_div(od, TD), ceil_div(oh, TH), ceil_div(ow, 16)


def deconv_ntiles(D, H, W, row):
    cin, cout, sd, TDM, THM = row
    return ceil_div(D, TDM), ceil_div(H, THM), ceil_div(W, 16)


# ---------------------------------------------------------------------------------------------------------------- operand models
def model_x(fmt, x):
    """The activations (or the skip tensor) a format's kernel contracts, as float64."""
    return (x.half() if fmt in F16_FORMATS else x).double()


def model_w(fmt, w):
    """The weights a format's kernel contracts, as float64."""
    if fmt == "f16x2":
        hi = w.to(torch.float16)
        lo = (w - hi.float()).to(torch.float16)
        return hi.double() + lo.double()
    if fmt == "f16":
        return w.half().double()
    return w.double()


def model_key(fmt):
    """Formats with the same key share one operand model (and so one float64 reference)."""
    return fmt if fmt in F16_FORMATS else "fp32"


def two_term_bf16(t):
    """t rounded to hi + lo bf16 (what the split-bf16 kernels contract), as float64."""
    s = packing.split_bf16(t.float())
    return s[0].double() + s[1].double()


# ---------------------------------------------------------------------------------------------------------------- the operations
def _ncdhw(t):
    return t.permute(0, 4, 1, 2, 3)


def _cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def conv(x, w, bias, stride, relu=True):
    """x [B,D,H,W,Cin], w [Cout,Cin,kd,3,3], bias [>= Cout] -> (y [B,OD,OH,OW,Cout], S) in float64: Conv3d with padding (kd//2,1,1)
    + bias + optional ReLU, and S = the same convolution of |x| with |w| (no bias)."""
    x, w = x.double(), w.double()
    pad = (w.shape[2] // 2, 1, 1)
    y = F.conv3d(_ncdhw(x), w, bias[:w.shape[0]].double(), stride=stride, padding=pad)
    s = F.conv3d(_ncdhw(x.abs()), w.abs(), None, stride=stride, padding=pad)
    return _cl(F.relu(y) if relu else y), _cl(s)


def deconv(x, w, bias, sd, relu=True, skip=None):
    """x [B,D,H,W,Cin], w [Cin,Cout,3,3,3] -> (y [B,sd*D,2H,2W,Cout], S): ConvTranspose3d(stride (sd,2,2), padding 1, output_padding
    (sd-1,1,1)) + bias + optional ReLU, THEN + skip."""
    x, w = x.double(), w.double()
    kw = dict(stride=(sd, 2, 2), padding=1, output_padding=(sd - 1, 1, 1))
    y = F.conv_transpose3d(_ncdhw(x), w, bias[:w.shape[1]].double(), **kw)
    s = F.conv_transpose3d(_ncdhw(x.abs()), w.abs(), None, **kw)
    y = _cl(F.relu(y) if relu else y)
    if skip is not None:
        y = y + skip.double()
    return y, _cl(s)


def prob_head(y, prob_w, prob_b):
    """The fused 1x1x1 head of the last U-Net layer: y [B,D,H,W,8] (after the skip add) -> logits [B,D,H,W] = sum_c y[c] prob_w[c] +
    prob_b, and A = sum_c |y[c] prob_w[c]|."""
    t = y.double() * prob_w.double()
    return t.sum(-1) + prob_b.double()[0], t.abs().sum(-1)


def head3(x, w1):
    """The one-channel 3x3x3 head: x [B,D,H,W,8], w1 [8,3,3,3] -> (logits [B,D,H,W], S)."""
    y, s = conv(x, w1[None], torch.zeros(1), (1, 1, 1), relu=False)
    return y[..., 0], s[..., 0]


def conv_products(row):
    """K of a conv row: products per output element."""
    return row[2] * 9 * row[0]


def deconv_products(row):
    """K of a transposed row: the largest tap count of a parity class (2 x 2 x 2 at depth stride 2, 3 x 2 x 2 at 1) times Cin."""
    return max(len(c) for c in packing.deconv_class_taps(row[2])) * row[0]


# ---------------------------------------------------------------------------------------------------------------- figures and bars
LAYER_BAR = 3e-5          # the project's bar for split-bf16 arithmetic (tests/test_fpn.py, test_fmt.py, test_vit.py)
F16_BITS_CAP = 0.02       # share of fp16 outputs that may differ from the once-rounded reference (test_feature_heads' cap)


def split_figure(got, ref):
    """max |got - ref| / max(1, max |ref|): the figure LAYER_BAR bounds."""
    return float((got.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def chain_figure(got, ref, S, K, rel=None):
    """max over the elements of |got - ref| / (rel + K 2^-24 S): <= 1 inside the bar.  rel = None: the fp32 bar K 2^-24 S; the fp16
    stores pass rel = 2^-11 |ref| (half an fp16 ulp of the stored value), the fused head 2^-11 sum_c |y_c prob_w_c|."""
    bound = K * 2.0 ** -24 * S
    if rel is not None:
        bound = bound + rel
    err = (got.double() - ref).abs()
    assert bool((bound[err > 0] > 0).all()), "an element with no products differs from the reference"
    return float((err / bound.clamp_min(1e-300)).max())


def f16_bits_share(got, ref):
    """Share of elements whose fp16 bits differ from fp16(ref) clamped to +-65504."""
    want = ref.clamp(-65504.0, 65504.0).to(torch.float16)
    return float((got.view(torch.int16) != want.view(torch.int16)).double().mean())
