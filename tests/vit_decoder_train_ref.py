"""TEST ORACLE: the reference's CrossVITDecoder (models/module.py:273-364) in TRAIN mode, fp64 by default and differentiable with torch
autograd.  The five blocks and the AAS mixing are tests/vit_decoder_ref.py's, reused by import (its `vit_decoder` is run for its captured
"tokens"; the eval-mode head it also computes is discarded); the head is restated here with F.batch_norm(training=True)'s semantics
written out, as tests/fpn_train_ref.py does: normalise with the batch mean and the biased variance over N H W, the running statistics
take one momentum step with the batch mean and the UNBIASED variance, num_batches_tracked grows by one.  Pinned to fixture F35 on the
CPU (tests/test_vit_decoder_train.py::test_oracle_pinned_to_f35).  Parameters and buffers come as a state dict with the reference's key names; pass fp64
leaf tensors that require grad to read the gradients off them."""
import torch
import torch.nn.functional as F

import vit_decoder_ref as R

BN_EPS = 1e-5
MOMENTUM = 0.1
HEAD = ("proj", "upsampler0", "upsampler1")


def _bn_silu_train(o, z, name, running):
    sd = o.sd
    mean = z.mean((0, 2, 3))
    var = ((z - mean.reshape(1, -1, 1, 1)) ** 2).mean((0, 2, 3))                       # biased: what normalises
    u = (z - mean.reshape(1, -1, 1, 1)) / torch.sqrt(var.reshape(1, -1, 1, 1) + BN_EPS) * R._p(sd, name + ".1.weight", z).reshape(1, -1, 1, 1) \
        + R._p(sd, name + ".1.bias", z).reshape(1, -1, 1, 1)
    if running is not None:
        m = z.numel() // z.shape[1]
        running[name + ".1.running_mean"] = (1 - MOMENTUM) * R._p(sd, name + ".1.running_mean", z).detach() + MOMENTUM * mean.detach()
        running[name + ".1.running_var"] = (1 - MOMENTUM) * R._p(sd, name + ".1.running_var", z).detach() + MOMENTUM * var.detach() * (m / max(m - 1, 1))
        running[name + ".1.num_batches_tracked"] = sd[name + ".1.num_batches_tracked"] + 1
    return F.silu(u)


def head_train(o, tokens, h, w, running=None):
    """tokens [N, h w, 768] -> proj -> upsampler0 -> upsampler1 -> [N, 64, 4 h, 4 w] with batch-statistics BatchNorm over all N views."""
    sd = o.sd
    t = tokens.reshape(tokens.shape[0], h, w, R.D).permute(0, 3, 1, 2)
    t = _bn_silu_train(o, F.conv2d(o.r(t), o.r(R._p(sd, "proj.0.weight", t)), R._p(sd, "proj.0.bias", t), padding=1), "proj", running)
    for name in HEAD[1:]:
        t = _bn_silu_train(o, F.conv_transpose2d(o.r(t), o.r(R._p(sd, name + ".0.weight", t)), R._p(sd, name + ".0.bias", t), stride=2, padding=1),
                           name, running)
    return t


def vit_decoder_train(x, sd, vit_shape, dtype=torch.float64, running=None, split_operands=False, capture=None):
    """x = three [B, V, h w, 768] tensors -> [B V, 64, 4 h, 4 w] in `dtype`, train mode; `running` (dict) receives the 6 updated running
    tensors and 3 num_batches_tracked; `capture` as vit_decoder_ref.vit_decoder's (blocks, refs, tokens)."""
    B, V, h, w, C = vit_shape
    cap = capture if capture is not None else {}
    R.vit_decoder(x, sd, vit_shape, dtype=dtype, capture=cap, split_operands=split_operands)       # its eval-mode head's output is discarded
    return head_train(R._Ops(sd, split_operands), cap["tokens"], h, w, running)
