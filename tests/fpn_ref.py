"""TEST ORACLE: a from-scratch torch-functional restatement of the reference's FPNEncoder / FPNDecoder (models/module.py:47-86,
200-270), computed in fp64 by default (fp32 where a test needs the whole full-size image fast).  Pinned to fixture F25 on the CPU
(tests/test_fpn.py); it is the oracle at sizes the fixture lacks.  Parameters come as a state dict with the reference's key names."""
import torch
import torch.nn.functional as F

ENC = (("conv00", 7, 1), ("conv01", 5, 1), ("downsample1", 5, 2), ("conv10", 3, 1), ("conv11", 3, 1), ("downsample2", 5, 2),
       ("conv20", 3, 1), ("conv21", 3, 1), ("downsample3", 3, 2), ("conv30", 3, 1), ("conv31", 3, 1))
BN_EPS = 1e-5


def _bn(y, sd, p):
    shape = (1, -1, 1, 1)
    m, v = sd[p + "running_mean"].to(y).reshape(shape), sd[p + "running_var"].to(y).reshape(shape)
    return (y - m) / torch.sqrt(v + BN_EPS) * sd[p + "weight"].to(y).reshape(shape) + sd[p + "bias"].to(y).reshape(shape)


def enc_layer(x, sd, name, k, stride, dtype=torch.float64):
    """Conv2d block (norm_type 'BN'): conv without bias -> BatchNorm (eval) -> leaky_relu(0.1)."""
    x = x.to(dtype)
    y = F.conv2d(x, sd[name + ".conv.weight"].to(x), None, stride, k // 2)
    return F.leaky_relu(_bn(y, sd, name + ".bn."), 0.1)


def head(x, sd, name, pad, dtype=torch.float64):
    """Sequential(Conv2d(bias), BatchNorm2d, Swish)."""
    x = x.to(dtype)
    y = _bn(F.conv2d(x, sd[name + ".0.weight"].to(x), sd[name + ".0.bias"].to(x), 1, pad), sd, name + ".1.")
    return y * torch.sigmoid(y)


def merge(prev, lat, sd, k, dtype=torch.float64):
    """up2(prev) (bilinear, align_corners=True) + inner_k(lat)."""
    prev, lat = prev.to(dtype), lat.to(dtype)
    up = F.interpolate(prev, scale_factor=2, mode="bilinear", align_corners=True)
    return up + F.conv2d(lat, sd["inner%d.weight" % k].to(lat), sd["inner%d.bias" % k].to(lat))


def encoder(x, sd, dtype=torch.float64, layers=None):
    """-> [conv01, conv11, conv21, conv31]; `layers` (dict) receives every layer's output."""
    t, outs = x, {}
    for name, k, s in ENC:
        t = enc_layer(t, sd, name, k, s, dtype)
        outs[name] = t
    if layers is not None:
        layers.update(outs)
    return [outs["conv01"], outs["conv11"], outs["conv21"], outs["conv31"]]


def decoder(conv01, conv11, conv21, conv31, sd, dtype=torch.float64, inter=None):
    """-> [out0, out1, out2, out3]; `inter` (dict) receives intra1 / intra2."""
    out0 = head(conv31, sd, "out0", 0, dtype)
    intra1 = merge(conv31, conv21, sd, 1, dtype)
    out1 = head(intra1, sd, "out1", 1, dtype)
    intra2 = merge(intra1, conv11, sd, 2, dtype)
    out2 = head(intra2, sd, "out2", 1, dtype)
    out3 = head(merge(intra2, conv01, sd, 3, dtype), sd, "out3", 1, dtype)
    if inter is not None:
        inter.update(intra1=intra1, intra2=intra2)
    return [out0, out1, out2, out3]
