"""The target loss of one run: which of the three rules (the cross-entropy, nanoGCG's mellowmax or the Carlini-Wagner
margin; EngineOptions.loss_rule) and the rule's parameter.  The kernels are behind ``ops``; nothing here touches a logit."""

from __future__ import annotations

import logging
from typing import Optional, Tuple

import torch

from . import ops
from .config import BimodalAttackConfig, EngineOptions, mellowmax_alpha

logger = logging.getLogger("gcg")


class TargetLoss:
    """One run's target loss.  `param`: alpha of "mellowmax" (config.mellowmax_alpha, the one rule that reads it: checked
    here, when the rule is selected), kappa of "margin" (it comes with the options, checked by from_env), None for "ce".
    `labels`: the (T,) int64 target ids, known once the prompt is."""

    def __init__(self, config: BimodalAttackConfig, opt: EngineOptions, labels: Optional[torch.Tensor] = None):
        self.rule, self.labels, self.param = opt.loss_rule, labels, None
        if self.rule == "mellowmax":
            self.param = mellowmax_alpha(config)
            logger.info(f"Target loss: mellowmax, alpha = {self.param} (loss_rule; the default is the cross-entropy)")
        elif self.rule == "margin":
            self.param = float(opt.margin_kappa)
            logger.info(f"Target loss: margin, kappa = {self.param} (loss_rule; the default is the cross-entropy)")

    def _labels(self) -> torch.Tensor:
        assert self.labels is not None, "TargetLoss: the labels come with the prompt, and none has been prepared"
        return self.labels

    def grad(self, logits: torch.Tensor) -> torch.Tensor:
        """Gradient pass: the (T, V) target rows of the one sequence -> the scalar loss, differentiable (the kernel's own
        dlogits)."""
        if self.rule == "margin":
            return ops.TargetMargin.apply(logits, self._labels(), self.param)
        if self.rule == "mellowmax":
            return ops.TargetMellowmax.apply(logits, self._labels(), self.param)
        return ops.TargetCrossEntropy.apply(logits, self._labels())

    def score(self, logits: torch.Tensor, want_hit: bool) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """Candidate scoring: (B, T, V) -> (loss (B,) fp32, early-stop hit or None).  The hit is the argmax test of the
        cross-entropy kernel's row pass under "ce" and "mellowmax" (there an extra pass, made only when it is wanted); the
        margin's own row pass finds each row's top-1 and returns the same test from its one read of the logits."""
        if self.rule == "margin":
            return ops.margin_target(logits, self._labels(), self.param, want_match=want_hit)[:2]
        if self.rule == "mellowmax":
            hit = ops.ce_target(logits, self._labels(), want_match=True)[1] if want_hit else None
            return ops.mellowmax_target(logits, self._labels(), self.param)[0], hit
        return ops.ce_target(logits, self._labels(), want_match=want_hit)[:2]
