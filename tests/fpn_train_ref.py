"""TEST ORACLE: a from-scratch torch-functional restatement of the reference's FPNDecoder (models/module.py:236-270) in TRAIN mode,
fp64 by default: every head is Conv2d (with bias) -> BatchNorm2d with batch statistics -> Swish, F.batch_norm(training=True)'s
semantics written out (normalise with the batch mean and the biased variance over N H W; the running statistics take one momentum
step with the batch mean and the UNBIASED variance).  Differentiable with torch autograd; pinned to fixture F33 on the CPU
(tests/test_fpn_train.py).  Parameters and buffers come as a state dict with the reference's key names."""
import torch
import torch.nn.functional as F

BN_EPS = 1e-5
MOMENTUM = 0.1
HEADS = (("out0", 0), ("out1", 1), ("out2", 1), ("out3", 1))           # name, padding
PARAMS = tuple("%s.%s" % (n, s) for n, _ in HEADS for s in ("0.weight", "0.bias", "1.weight", "1.bias")) + \
    tuple("inner%d.%s" % (k, s) for k in (1, 2, 3) for s in ("weight", "bias"))


def head(x, sd, name, pad, running=None):
    """Sequential(Conv2d(bias), BatchNorm2d (train mode), Swish) -> y; `running` (dict) receives the updated running statistics and
    num_batches_tracked of this head."""
    z = F.conv2d(x, sd[name + ".0.weight"].to(x), sd[name + ".0.bias"].to(x), 1, pad)
    mean = z.mean((0, 2, 3))
    var = ((z - mean.reshape(1, -1, 1, 1)) ** 2).mean((0, 2, 3))                       # biased: what normalises
    u = (z - mean.reshape(1, -1, 1, 1)) / torch.sqrt(var.reshape(1, -1, 1, 1) + BN_EPS) * sd[name + ".1.weight"].to(x).reshape(1, -1, 1, 1) \
        + sd[name + ".1.bias"].to(x).reshape(1, -1, 1, 1)
    if running is not None:
        m = z.numel() // z.shape[1]
        running[name + ".1.running_mean"] = (1 - MOMENTUM) * sd[name + ".1.running_mean"].to(x) + MOMENTUM * mean.detach()
        running[name + ".1.running_var"] = (1 - MOMENTUM) * sd[name + ".1.running_var"].to(x) + MOMENTUM * var.detach() * (m / max(m - 1, 1))
        running[name + ".1.num_batches_tracked"] = sd[name + ".1.num_batches_tracked"] + 1
    return u * torch.sigmoid(u)


def merge(prev, lat, sd, k):
    """up2(prev) (bilinear, align_corners=True) + inner_k(lat)."""
    up = F.interpolate(prev, scale_factor=2, mode="bilinear", align_corners=True)
    return up + F.conv2d(lat, sd["inner%d.weight" % k].to(lat), sd["inner%d.bias" % k].to(lat))


def decoder(conv01, conv11, conv21, conv31, sd, dtype=torch.float64, running=None):
    """-> [out0, out1, out2, out3] in train mode; `running` (dict) receives the 8 updated running tensors and 4 num_batches_tracked."""
    c01, c11, c21, c31 = (t.to(dtype) for t in (conv01, conv11, conv21, conv31))
    out0 = head(c31, sd, "out0", 0, running)
    intra1 = merge(c31, c21, sd, 1)
    out1 = head(intra1, sd, "out1", 1, running)
    intra2 = merge(intra1, c11, sd, 2)
    out2 = head(intra2, sd, "out2", 1, running)
    out3 = head(merge(intra2, c01, sd, 3), sd, "out3", 1, running)
    return [out0, out1, out2, out3]
