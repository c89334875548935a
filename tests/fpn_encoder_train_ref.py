"""TEST ORACLE: a from-scratch torch-functional restatement of the reference's FPNEncoder (models/module.py:47-86, 200-233, norm_type
'BN') in TRAIN mode, fp64 by default: each of the eleven blocks is Conv2d (no bias) -> BatchNorm2d with batch statistics ->
leaky_relu(0.1), F.batch_norm(training=True)'s semantics written out (normalise with the batch mean and the biased variance over N H W;
the running statistics take one momentum step with the batch mean and the UNBIASED variance).  Differentiable with torch autograd; pinned
to fixture F34 on the CPU (tests/test_fpn_encoder_train.py).  Parameters and buffers come as a state dict with the reference's key names."""
import torch
import torch.nn.functional as F

BN_EPS = 1e-5
MOMENTUM = 0.1
ENC = (("conv00", 7, 1), ("conv01", 5, 1), ("downsample1", 5, 2), ("conv10", 3, 1), ("conv11", 3, 1), ("downsample2", 5, 2),
       ("conv20", 3, 1), ("conv21", 3, 1), ("downsample3", 3, 2), ("conv30", 3, 1), ("conv31", 3, 1))
PARAMS = tuple("%s.%s" % (n, s) for n, _, _ in ENC for s in ("conv.weight", "bn.weight", "bn.bias"))
OUTPUTS = ("conv01", "conv11", "conv21", "conv31")


def bn_leaky(z, gamma, beta, pre=None):
    """Batch-statistics BatchNorm2d + leaky_relu(0.1) of z -> (y, batch mean, biased variance); `pre` (list) receives the normalised
    pre-activation u = gamma xhat + beta."""
    shape = (1, -1, 1, 1)
    mean = z.mean((0, 2, 3))
    var = ((z - mean.reshape(shape)) ** 2).mean((0, 2, 3))                             # biased: what normalises
    u = (z - mean.reshape(shape)) / torch.sqrt(var.reshape(shape) + BN_EPS) * gamma.to(z).reshape(shape) + beta.to(z).reshape(shape)
    if pre is not None:
        pre.append(u.detach())
    return F.leaky_relu(u, 0.1), mean, var


def block(x, sd, name, k, stride, running=None, pre=None):
    """One Conv2d block in train mode -> y; `running` (dict) receives the block's updated running statistics and num_batches_tracked,
    `pre` (dict) its normalised pre-activation u under `name`."""
    z = F.conv2d(x, sd[name + ".conv.weight"].to(x), None, stride, k // 2)
    us = [] if pre is not None else None
    y, mean, var = bn_leaky(z, sd[name + ".bn.weight"], sd[name + ".bn.bias"], us)
    if pre is not None:
        pre[name] = us[0]
    if running is not None:
        m = z.numel() // z.shape[1]
        running[name + ".bn.running_mean"] = (1 - MOMENTUM) * sd[name + ".bn.running_mean"].to(x) + MOMENTUM * mean.detach()
        running[name + ".bn.running_var"] = (1 - MOMENTUM) * sd[name + ".bn.running_var"].to(x) + MOMENTUM * var.detach() * (m / max(m - 1, 1))
        running[name + ".bn.num_batches_tracked"] = sd[name + ".bn.num_batches_tracked"] + 1
    return y


def encoder(x, sd, dtype=torch.float64, running=None, pre=None):
    """-> [conv01, conv11, conv21, conv31] in train mode; `running` (dict) receives the 22 updated running tensors and 11
    num_batches_tracked, `pre` (dict) every block's normalised pre-activation u."""
    t, outs = x.to(dtype), {}
    for name, k, s in ENC:
        t = block(t, sd, name, k, s, running, pre)
        outs[name] = t
    return [outs[n] for n in OUTPUTS]
