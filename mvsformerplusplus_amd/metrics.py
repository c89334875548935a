"""The validation metrics on the device (utils.py:156-189 and trainer/mvsformer_trainer.py:288-336).

``Thres_metrics`` and ``AbsDepthError_metrics`` keep the reference's signatures; ``validation_metrics`` returns the eight entries that
``_valid_epoch`` builds from them out of ONE metrics launch (plus its finalize), as zero-dim device tensors and without a host
synchronisation; ``ValidationMeter`` accumulates them on the device and synchronises once, in ``mean()``.

The reference's conventions, per image and then averaged over the images of the batch:
  * ``Thres_metrics`` of an image with no valid pixel is NaN (a mean over nothing) and poisons the batch mean;
  * ``AbsDepthError_metrics`` of an empty band is 0; without a band over no valid pixel it is NaN.
The reference multiplies ``depth_interval[j].item()`` (divided by 2.65 on the DTU branch) in Python doubles and compares the double with a
fp32 tensor, for which torch rounds the scalar to fp32: the kernel forms the same fp64 products from the fp32 interval on the device, rounds
them to fp32 and compares fp32 with fp32.  There is no CPU route: host tensors raise ``MvsHipError``.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import ops

__all__ = ["Thres_metrics", "AbsDepthError_metrics", "validation_metrics", "ValidationMeter", "VALIDATION_KEYS"]

_MM = (2, 4, 8, 14)
VALIDATION_KEYS = tuple("abs_depth_thres0-%dmm_error" % k for k in _MM) + tuple("thres%dmm_error" % k for k in _MM)


def _maps(depth_est, depth_gt, mask):
    est, gt = (t.detach() if t.dtype == torch.float32 else t.detach().float() for t in (depth_est, depth_gt))
    if mask.dtype not in (torch.float32, torch.bool, torch.uint8):
        mask = mask.float()
    return est, gt, mask.detach()


def Thres_metrics(depth_est, depth_gt, mask, thres) -> torch.Tensor:
    """utils.py:169-176: the share of the valid pixels with |est - gt| > thres per image, averaged over the images ([B,H,W] maps; mask
    bool, or fp32 taken as > 0.5).  A zero-dim device tensor."""
    assert isinstance(thres, (int, float))
    _, _, means = ops.depth_metrics(*_maps(depth_est, depth_gt, mask), [float(thres)], [None])
    return means[-1, 0]


def AbsDepthError_metrics(depth_est, depth_gt, mask, thres=None) -> torch.Tensor:
    """utils.py:180-189: the mean |est - gt| over the valid pixels per image, restricted to thres[0] <= error <= thres[1] when ``thres`` is
    given (an empty band: 0), averaged over the images.  A zero-dim device tensor."""
    band = None if thres is None else (float(thres[0]), float(thres[1]))
    _, _, means = ops.depth_metrics(*_maps(depth_est, depth_gt, mask), [0.0], [band])
    return means[-1, 1]


def validation_metrics(depth_est, depth_gt, mask, depth_interval, blended: bool = False) -> Dict[str, torch.Tensor]:
    """The eight entries of ``_valid_epoch`` (mvsformer_trainer.py:288-314) as zero-dim device tensors: ``abs_depth_thres0-{2,4,8,14}mm_error``
    and ``thres{2,4,8,14}mm_error``.  ``depth_interval`` fp32 [B]; ``blended=True`` is the BlendedLoader branch (every sample against its own
    interval, the mean over the samples), otherwise ``depth_interval[0] / 2.65`` serves the whole batch.  ``mask`` is the stage's mask (fp32,
    taken as > 0.5) or a bool map."""
    interval = depth_interval.detach().reshape(-1)
    if interval.dtype != torch.float32:
        interval = interval.float()
    factors = [float(k) for k in _MM]
    _, _, means = ops.depth_metrics(*_maps(depth_est, depth_gt, mask), factors, [(0.0, f) for f in factors], interval=interval,
                                    divisor=1.0 if blended else 2.65, per_sample=bool(blended))
    row, T = means[-1], len(_MM)
    out = {VALIDATION_KEYS[i]: row[T + i] for i in range(T)}
    out.update({VALIDATION_KEYS[T + i]: row[i] for i in range(T)})
    return out


class ValidationMeter:
    """``DictAverageMeter`` for device scalars: ``update`` adds a dictionary of zero-dim tensors on the device, ``mean()`` synchronises once
    and appends ``mean_error``, the average of the four ``thres*`` entries, as ``_valid_epoch`` does (mvsformer_trainer.py:333-336)."""

    def __init__(self):
        self.reset()

    def reset(self) -> None:
        self.keys, self.total, self.count = None, None, 0

    def update(self, values: Dict[str, torch.Tensor], n: int = 1) -> None:
        if self.keys is None:
            self.keys = list(values)
        elif list(values) != self.keys:
            raise ValueError("ValidationMeter.update: the keys changed from %s to %s" % (self.keys, list(values)))
        row = torch.stack([values[k].detach().reshape(()).double() for k in self.keys])
        self.total = row if self.total is None else self.total + row
        self.count += n

    def mean(self) -> Dict[str, float]:
        if self.total is None:
            return {}
        out = {k: v / self.count for k, v in zip(self.keys, self.total.tolist())}        # the one synchronisation
        if all("thres%dmm_error" % k in out for k in _MM):
            out["mean_error"] = sum(out["thres%dmm_error" % k] for k in _MM) / 4.0
        return out
