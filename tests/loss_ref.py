"""TEST INFRASTRUCTURE: the inputs of the loss / metric cases and a restatement of the losses in torch, written from the contract in
DESIGN.md section 4.16 (never from the reference's text).

Inputs are built from an exact integer hash (24-bit values, int64 arithmetic without overflow) and exactly rounded elementwise fp64 -> fp32
operations, so that every machine and torch version regenerates the bits the fixture tests/golden/f30_losses.npz was recorded on; the
fixture pins a checksum of every case's inputs.

The restatement takes the DECISIONS (bin index, range tests, masks) in fp32, as the kernels and the reference do, and everything after them
in the dtype asked for: float64 is the yardstick, float32 is "the composite" whose own distance from the yardstick sets the bars."""
import numpy as np
import torch
import torch.nn.functional as F


# ---- deterministic inputs ---------------------------------------------------------------------------------------------------------
def hash24(n, seed):
    """n pseudo-random integers in [0, 2^24) as int64 (every product stays below 2^56)."""
    h = (torch.arange(n, dtype=torch.int64) * 1103515245 + 12345 + int(seed) * 40503) % (1 << 24)
    for mult, shift in ((1664525, 11), (22695477, 7), (69069, 13)):
        h = (h * mult + 1013904223) % (1 << 24)
        h = h ^ (h >> shift)
    return h


def uniform(shape, seed):
    """fp64 in [0, 1) with 24-bit resolution (exact in fp32)."""
    n = int(np.prod(shape))
    return (hash24(n, seed).double() / float(1 << 24)).reshape(shape)


def ascending(hyp, inverse):
    return hyp.flip(1) if inverse else hyp


def intervals(d):
    iv = (d[:, 1:] - d[:, :-1]).abs() / 2
    return torch.cat([iv, iv[:, -1:]], 1)


def make_hyp(B, D, H, W, inverse, seed):
    """Hypotheses that vary per pixel, unevenly spaced; stored from far to near when inverse."""
    start = 400.0 + 100.0 * uniform((B, 1, H, W), seed + 1)
    step = 2.0 + 2.0 * uniform((B, 1, H, W), seed + 2)
    curv = 0.05 * uniform((B, 1, H, W), seed + 3)
    k = torch.arange(D, dtype=torch.float64).reshape(1, D, 1, 1)
    d = (start + step * k + curv * (k * k)).float()
    return d.flip(1).contiguous() if inverse else d


def make_gt_mask(hyp, inverse, seed, mask_mode="mixed"):
    """Ground truth by category: below the first bin, above the last, exactly on a plane, exactly on a bin edge d + iv, exactly on the lower
    end d[0] - iv[0], the rest inside the range.  mask in {0, 0.5, 1} (0.5 is excluded by > 0.5); mask_mode "zero" = all zero,
    "image0" = image 0 all zero."""
    B, D, H, W = hyp.shape
    d = ascending(hyp, inverse)
    iv = intervals(d)
    cat = (hash24(B * H * W, seed + 4) % 8).reshape(B, H, W)
    kk = (hash24(B * H * W, seed + 5) % D).reshape(B, 1, H, W)
    u = uniform((B, H, W), seed + 6).float()
    on_plane = d.gather(1, kk).squeeze(1)
    on_edge = (d + iv).gather(1, kk).squeeze(1)
    lower = d[:, 0] - iv[:, 0]
    upper = d[:, -1] + iv[:, -1]
    gt = d[:, 0] + u * (d[:, -1] - d[:, 0])
    gt = torch.where(cat == 0, lower - 0.5 - u, gt)
    gt = torch.where(cat == 1, upper + 0.5 + u, gt)
    gt = torch.where(cat == 2, on_plane, gt)
    gt = torch.where(cat == 3, on_edge, gt)
    gt = torch.where(cat == 4, lower, gt)
    m = (hash24(B * H * W, seed + 7) % 4).reshape(B, H, W)
    mask = torch.where(m == 0, 0.0, torch.where(m == 1, 0.5, 1.0)).float()
    if mask_mode == "zero":
        mask = torch.zeros_like(mask)
    elif mask_mode == "image0":
        mask[0] = 0.0
    return gt.contiguous(), mask.contiguous()


# name -> (B, D, H, W, inverse, mask_mode).  13 x 23: W odd, fewer pixels than one workgroup; 37 x 67: several workgroups and a partly filled
# last one.  D = 2 is the smallest accepted, 5 is odd, 32 the shipped maximum.
CE_CASES = {
    "d2": (2, 2, 13, 23, False, "mixed"), "d2i": (2, 2, 13, 23, True, "mixed"),
    "d4": (2, 4, 13, 23, False, "mixed"), "d4i": (2, 4, 37, 67, True, "mixed"),
    "d5": (2, 5, 37, 67, False, "mixed"), "d5i": (2, 5, 13, 23, True, "mixed"),
    "d32": (2, 32, 13, 23, False, "mixed"), "d32i": (2, 32, 13, 23, True, "mixed"),
    "zero": (2, 4, 13, 23, True, "zero"), "image0": (2, 5, 13, 23, False, "image0"),
}
CE_WEIGHT = 1.5


def ce_inputs(name):
    B, D, H, W, inverse, mode = CE_CASES[name]
    seed = 1000 + 37 * sorted(CE_CASES).index(name)
    hyp = make_hyp(B, D, H, W, inverse, seed)
    gt, mask = make_gt_mask(hyp, inverse, seed, mode)
    logits = (uniform((B, D, H, W), seed + 8) * 8.0 - 4.0).float()
    return {"logits": logits, "hyp": hyp, "gt": gt, "mask": mask, "inverse": inverse}


# name -> (B, D, H, W, inverse, mask_mode): the "reg" loss with per-sample intervals, without and with the dynamic clamp
REG_CASES = {"r13": (2, 4, 13, 23, True, "mixed"), "r37": (2, 5, 37, 67, False, "mixed"), "rzero": (2, 4, 13, 23, False, "zero")}
REG_WEIGHT = 2.0


def reg_inputs(name):
    B, D, H, W, inverse, mode = REG_CASES[name]
    seed = 5000 + 41 * sorted(REG_CASES).index(name)
    hyp = make_hyp(B, D, H, W, inverse, seed)
    gt, mask = make_gt_mask(hyp, inverse, seed, mode)
    interval = torch.tensor([2.5, 1.06 * 2.5])[:B].float()
    # errors from well inside the quadratic part to several hypothesis ranges (so that the clamp fires on some pixels and not on others)
    spread = torch.where(hash24(B * H * W, seed + 9).reshape(B, H, W) % 3 == 0, 40.0, 3.0)
    depth = (gt.double() + (uniform((B, H, W), seed + 10) - 0.5) * spread).float()
    return {"depth": depth, "hyp": hyp, "gt": gt, "mask": mask, "interval": interval, "inverse": inverse}


MS_STAGES = {"stage1": (32, 5, 7), "stage2": (16, 7, 9), "stage3": (8, 9, 11), "stage4": (4, 13, 23)}
MS_TYPES = ["ce", "ce", "reg", "ce"]
MS_ARGS = {"dlossw": [1.0, 0.5, 2.0, 1.5], "clip_func": "dynamic"}


def multi_stage_inputs():
    """A four-stage output dictionary (B = 2, inverse depth) with its ground truths, masks and intervals."""
    outputs, gts, masks = {}, {}, {}
    for i, (key, (D, H, W)) in enumerate(MS_STAGES.items()):
        seed = 9000 + 53 * i
        hyp = make_hyp(2, D, H, W, True, seed)
        gt, mask = make_gt_mask(hyp, True, seed)
        logits = (uniform((2, D, H, W), seed + 8) * 8.0 - 4.0).float()
        depth = (gt.double() + (uniform((2, H, W), seed + 10) - 0.5) * 6.0).float()
        outputs[key] = {"depth": depth, "depth_values": hyp, "prob_volume_pre": logits}
        gts[key], masks[key] = gt, mask
    return outputs, gts, masks, torch.tensor([2.5, 2.65]).float()


# name -> (B, H, W, mask_mode)
METRIC_CASES = {"m13": (2, 13, 23, "mixed"), "m37": (2, 37, 67, "mixed"), "mimage0": (2, 13, 23, "image0"), "mzero": (2, 13, 23, "zero")}
MM = (2, 4, 8, 14)


def metric_thresholds(interval, blended):
    """fp32 thresholds [B, 4] as the reference's comparisons see them: the fp64 product of Python scalars rounded to fp32."""
    itv = interval.double().numpy()
    rows = [[np.float32((itv[b] if blended else itv[0] / 2.65) * k) for k in MM] for b in range(len(itv))]
    return np.asarray(rows, dtype=np.float32)


def metric_inputs(name):
    """Errors spread over all bands, plus, in every image, pixels (ground truth 0, so that |est - gt| is the planted value exactly) whose
    error is a threshold of either form or one fp32 ulp on either side of it, and exact zeros (the lower band end)."""
    B, H, W, mode = METRIC_CASES[name]
    seed = 7000 + 43 * sorted(METRIC_CASES).index(name)
    interval = torch.tensor([2.5, 2.5 * 1.06])[:B].float()
    gt = (425.0 + 500.0 * uniform((B, H, W), seed + 1)).float()
    err = (uniform((B, H, W), seed + 2) - 0.5) * 2.0 * 16.0 * 2.5
    est = (gt.double() + err).float()
    planted = sorted({float(v) for blended in (False, True) for t in metric_thresholds(interval, blended).reshape(-1)
                      for v in (np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1e9)))} | {0.0})
    assert len(planted) + 3 <= H * W
    m = (hash24(B * H * W, seed + 3) % 4).reshape(B, H, W)
    mask = torch.where(m == 0, 0.0, torch.where(m == 1, 0.5, 1.0)).float()
    ev, gv, mv = est.view(B, -1), gt.view(B, -1), mask.view(B, -1)
    for b in range(B):
        for i, v in enumerate(planted):
            gv[b, 3 + i] = 0.0
            ev[b, 3 + i] = v if i % 2 else -v
            mv[b, 3 + i] = 1.0
        ev[b, 0] = gv[b, 0]                       # an exact zero error at a non-zero depth
        mv[b, 0] = 1.0
    if mode == "zero":
        mask = torch.zeros_like(mask)
    elif mode == "image0":
        mask[0] = 0.0
    return {"est": est.contiguous(), "gt": gt.contiguous(), "mask": mask.contiguous(), "interval": interval}


def checksum(inputs):
    """One fp64 number per case: the position-weighted sum of every tensor's values (exact inputs give an exact match)."""
    total = 0.0
    for k in sorted(inputs):
        v = inputs[k]
        if torch.is_tensor(v):
            flat = v.double().reshape(-1)
            total += float((flat * (1.0 + (torch.arange(flat.numel(), dtype=torch.float64) % 7))).sum())
    return total


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def ce_decisions(hyp, gt, mask, inverse):
    """fp32: (bin index in WALK order, int64 [B,H,W]; valid bool [B,H,W])."""
    d = ascending(hyp.float(), inverse)
    D = d.shape[1]
    iv = intervals(d)
    g = gt.float().unsqueeze(1)
    index = ((d + iv) <= g).sum(1).clamp_max(D - 1)
    outside = (g < d[:, 0:1] - iv[:, 0:1]) | (g > d[:, -1:] + iv[:, -1:])
    return index, (~outside.squeeze(1)) & (mask > 0.5)


def stored_index(index, valid, D, inverse):
    """Walk-order bins -> the kernel's convention: the plane in stored order, -1 where not valid."""
    k = (D - 1 - index) if inverse else index
    return torch.where(valid, k, torch.full_like(k, -1)).to(torch.int32)


def ce_value(logits, hyp, gt, mask, inverse, weight, dtype):
    """weight * mean cross entropy over the valid pixels, computed in `dtype` after the fp32 decisions; `logits` may require grad."""
    index, valid = ce_decisions(hyp, gt, mask, inverse)
    x = ascending(logits.to(dtype), inverse).permute(0, 2, 3, 1)[valid]
    if x.shape[0] == 0:
        return weight * (x.sum() + float("nan"))                  # a mean over nothing
    return weight * F.cross_entropy(x, index[valid], reduction="mean")


def reg_value(depth, gt, mask, interval, hyp, inverse, weight, dtype):
    """weight * mean smooth L1 (beta 1) of depth / interval over mask > 0.5, clamped from above by the hypotheses' range / interval when
    `hyp` is given; interval None = 1."""
    valid = mask > 0.5
    itv = torch.ones(depth.shape[0], dtype=dtype) if interval is None else interval.to(dtype)
    itv = itv.reshape(-1, 1, 1)
    e, t = depth.to(dtype) / itv, gt.to(dtype) / itv
    loss = F.smooth_l1_loss(e[valid], t[valid], reduction="none")
    if hyp is not None:
        d = ascending(hyp.to(dtype), inverse)
        loss = torch.clamp_max(loss, ((d[:, -1] - d[:, 0]) / itv)[valid])
    return weight * loss.mean()


def value_and_grad(fn, leaf, dtype):
    """fn(leaf in dtype, requiring grad) -> (value as a Python float, gradient in fp64)."""
    x = leaf.detach().to(dtype).requires_grad_(True)
    v = fn(x)
    g = torch.autograd.grad(v, x)[0] if bool(torch.isfinite(v)) else torch.zeros_like(x)
    return float(v.detach()), g.double()


def loss_bar(ref, composite):
    """Four times the fp32 composite's own distance from the fp64 value, with a floor of 2^-22 relative."""
    return max(4.0 * abs(composite - ref), 2.0 ** -22 * abs(ref))


def grad_bar(ref, composite):
    """Elementwise: the larger of four times the composite's own error and 1e-6 of max |grad|."""
    return torch.maximum(4.0 * (composite - ref).abs(), 1e-6 * ref.abs().max().expand_as(ref))
