"""The multi-stage depth losses on the device (models/losses.py).

``get_multi_stage_losses``, ``get_loss``, ``ce_loss``, ``reg_loss`` and ``simple_loss`` keep the reference's signatures and return
dictionaries.  Every stage's loss is a ``torch.autograd.Function`` over the kernels of csrc/loss_kernels.hip: two launches forward (the
per-pixel pass and the ordered sum of its partials), one backward, no composite op over a volume and no host synchronisation.  Gradients
flow to ``prob_volume_pre`` ("ce") or ``depth`` ("reg") only; ``depth_values``, the ground truth, the masks and the intervals are constants
(the reference's comparisons and boolean indexing cut the graph there as well).  They accept the output dictionaries of the native
``StageNet`` in train mode and of the reference model alike.  There is no CPU route: host tensors raise ``MvsHipError``.

Quirks of the reference that are restated on purpose:
  * ``ce_loss`` returns ONLY THE LAST stage's entry: the block that fills the dictionary is dedented out of its loop (losses.py:191-195);
  * ``ce_loss`` accepts ``focal`` / ``gamma`` and ignores them;
  * ``get_multi_stage_losses`` asserts ``len(stage_keys) == len(depth_types)`` and ``depth_type in ("ce", "reg")``;
  * a loss over no valid pixel is NaN (a mean over nothing), and its gradient is all zeros.
The ``log_var`` (uncertainty) form of the "reg" loss is not built and raises ``NotImplementedError``.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import ops

__all__ = ["get_multi_stage_losses", "get_loss", "ce_loss", "reg_loss", "simple_loss"]

STAGE_KEYS = ("stage1", "stage2", "stage3", "stage4")


def _const32(t: torch.Tensor) -> torch.Tensor:
    return t.detach() if t.dtype == torch.float32 else t.detach().float()


class _CrossEntropyStage(torch.autograd.Function):
    """weight * mean over the valid pixels of -log softmax(logits)[bin of gt]; keeps index and lse (8 bytes per pixel) for the backward."""

    @staticmethod
    def forward(ctx, logits, hyp, gt, mask, inverse, weight):
        x = logits.detach().contiguous()
        loss, count, index, lse = ops.ce_loss_fwd(x, hyp, gt, mask, inverse, weight)
        ctx.save_for_backward(x, index, lse, count)
        ctx.weight = weight
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        x, index, lse, count = ctx.saved_tensors
        return ops.ce_loss_bwd(x, index, lse, grad_loss, count, ctx.weight), None, None, None, None, None


class _RegressionStage(torch.autograd.Function):
    """weight * mean over mask > 0.5 of smooth L1 (beta 1) on depth / interval, optionally clamped by the hypotheses' range; the backward
    recomputes the pixel from the inputs."""

    @staticmethod
    def forward(ctx, depth, gt, mask, interval, hyp, inverse, weight):
        d = depth.detach().contiguous()
        loss, count = ops.reg_loss_fwd(d, gt, mask, interval, hyp, inverse, weight)
        ctx.save_for_backward(d, gt, mask, count, *[t for t in (interval, hyp) if t is not None])
        ctx.has = (interval is not None, hyp is not None)
        ctx.inverse, ctx.weight = inverse, weight
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        d, gt, mask, count, *rest = ctx.saved_tensors
        interval = rest.pop(0) if ctx.has[0] else None
        hyp = rest.pop(0) if ctx.has[1] else None
        return ops.reg_loss_bwd(d, gt, mask, interval, hyp, ctx.inverse, grad_loss, count, ctx.weight), None, None, None, None, None, None


def _weight(dlossw, stage_key: str) -> float:
    return 1.0 if dlossw is None else float(dlossw[int(stage_key.replace("stage", "")) - 1])


def _ce_stage(stage_inputs, depth_gt, mask, inverse_depth, weight: float) -> torch.Tensor:
    logits = stage_inputs["prob_volume_pre"].float()              # 16-bit logits under autocast are cast, as losses.py:33 does
    return _CrossEntropyStage.apply(logits, _const32(stage_inputs["depth_values"]), _const32(depth_gt), _const32(mask), bool(inverse_depth),
                                    weight)


def _reg_stage(depth, depth_gt, mask, depth_interval, hyp, inverse_depth, weight: float) -> torch.Tensor:
    interval = None if depth_interval is None else _const32(depth_interval).reshape(-1)
    return _RegressionStage.apply(depth.float(), _const32(depth_gt), _const32(mask), interval, None if hyp is None else _const32(hyp),
                                  bool(inverse_depth), weight)


def get_multi_stage_losses(loss_args, depth_types: Sequence[str], outputs, depth_gt_ms, mask_ms, depth_interval,
                           inverse_depth) -> Dict[str, torch.Tensor]:
    """losses.py:19-101: {stage key: dlossw[stage] * loss} over the stages present in ``outputs``; ``depth_types[stage]`` is "ce" (cross
    entropy of ``prob_volume_pre`` against the bin of ``depth_values`` that holds the ground truth) or "reg" (smooth L1 of ``depth`` in
    units of ``depth_interval`` [B], clamped by the hypotheses' range when ``loss_args["clip_func"] == "dynamic"``)."""
    depth_loss_weights = loss_args["dlossw"]
    loss_dict = {}
    stage_keys = [k for k in STAGE_KEYS if k in outputs]
    assert len(stage_keys) == len(depth_types)
    for stage_key in stage_keys:
        stage_inputs = outputs[stage_key]
        depth_type = depth_types[int(stage_key.replace("stage", "")) - 1]
        assert depth_type in ("ce", "reg")
        weight = _weight(depth_loss_weights, stage_key)
        if depth_type == "ce":
            loss_dict[stage_key] = _ce_stage(stage_inputs, depth_gt_ms[stage_key], mask_ms[stage_key], inverse_depth, weight)
        else:
            if stage_inputs.get("log_var", None) is not None:
                raise NotImplementedError("the log_var (uncertainty) form of the 'reg' loss is not built: no shipped config produces log_var")
            hyp = stage_inputs["depth_values"] if loss_args.get("clip_func", None) == "dynamic" else None
            loss_dict[stage_key] = _reg_stage(stage_inputs["depth"], depth_gt_ms[stage_key], mask_ms[stage_key], depth_interval, hyp,
                                              inverse_depth, weight)
    return loss_dict


def get_loss(loss_arg, depth_type, outputs, depth_gt_ms_tmp, mask_ms_tmp, depth_interval, inverse_depth) -> Dict[str, torch.Tensor]:
    """losses.py:104-115: "re" -> reg_loss, "ce" -> ce_loss (the last stage only, see there), both with unit stage weights."""
    if depth_type == "re":
        return reg_loss(outputs, depth_gt_ms_tmp, mask_ms_tmp, dlossw=[1, 1, 1, 1], depth_interval=depth_interval)
    if depth_type == "ce":
        return ce_loss(outputs, depth_gt_ms_tmp, mask_ms_tmp, dlossw=[1, 1, 1, 1], focal=loss_arg["focal"], gamma=loss_arg["gamma"],
                       inverse_depth=inverse_depth)
    raise NotImplementedError(f"Unknown loss {depth_type}")


def simple_loss(outputs, depth_gt_ms, mask_ms) -> torch.Tensor:
    """losses.py:118-125: the smooth L1 mean of ``outputs["depth"]`` against one ground-truth map over mask > 0.5."""
    return _reg_stage(outputs["depth"], depth_gt_ms, mask_ms, None, None, False, 1.0)


def reg_loss(inputs, depth_gt_ms, mask_ms, dlossw, depth_interval) -> Dict[str, torch.Tensor]:
    """losses.py:128-149: the smooth L1 mean of depth / interval per stage that has a ground truth (``inputs`` holds all four stages, as in
    the reference); ``dlossw`` None leaves the stages unweighted."""
    loss_dict = {}
    for stage_key in STAGE_KEYS:
        stage_inputs = inputs[stage_key]
        if stage_key not in depth_gt_ms:
            continue
        loss_dict[stage_key] = _reg_stage(stage_inputs["depth"], depth_gt_ms[stage_key], mask_ms[stage_key], depth_interval, None, False,
                                          _weight(dlossw, stage_key))
    return loss_dict


def ce_loss(inputs, depth_gt_ms, mask_ms, dlossw, focal=False, gamma=0.0, inverse_depth=True) -> Dict[str, torch.Tensor]:
    """losses.py:152-197.  Returns ONLY THE LAST stage's entry, as the reference does (its final block sits outside the loop: a two-stage call
    returns ``['stage2']``), so only that stage is computed.  ``focal`` and ``gamma`` are accepted and ignored, as in the reference."""
    stage_keys = [k for k in STAGE_KEYS if k in inputs]
    if not stage_keys:
        raise ValueError("ce_loss: no stage1 .. stage4 entry in the inputs")
    stage_key = stage_keys[-1]
    return {stage_key: _ce_stage(inputs[stage_key], depth_gt_ms[stage_key], mask_ms[stage_key], inverse_depth, _weight(dlossw, stage_key))}
