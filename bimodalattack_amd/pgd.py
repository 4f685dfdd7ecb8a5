"""The image update of one run: which of the four rules (plain PGD or the reference's auto-PGD, in the L-inf box or the L2
ball) and everything the run keeps for it between steps.  The kernels are behind ``ops``; nothing here touches a pixel."""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops


class ApgdState:
    """What the reference's perform_autopgd_step keeps between calls (:1052-1061), for ONE run: eta, the best loss, the
    loss at the last checkpoint and the improvement count as Python floats / ints (as the reference keeps them), and the
    previous and best images as device buffers that only the kernel writes.  `decide` turns the call's (current_loss,
    step index) into the kernel's flags without touching the device."""

    MOMENTUM, RHO, INTERVAL = 0.75, 0.75, 10

    def __init__(self, eps: float, norm: str = "linf"):
        if norm not in ("linf", "l2"):
            raise ValueError(f"ApgdState: norm must be 'linf' or 'l2', got {norm!r}")
        self.eps = eps
        self.norm = norm                      # "l2": the ball instead of the box (bma_apgd_l2_step); decide() is the same
        self.started = False
        self.eta = 2 * eps                    # initial step size (:1058); config.alpha is not used
        self.best_loss = float("inf")
        self.last_best = float("inf")
        self.count = 0
        self.prev: Optional[torch.Tensor] = None
        self.best: Optional[torch.Tensor] = None
        self.last = None                      # (eta, take_best, restart) of the latest call

    def decide(self, current_loss: Optional[float], i: int) -> Tuple[float, bool, bool]:
        """(eta of this call's descent step, take_best, restart); advances the host state as the reference's call does."""
        if not self.started:
            self.started = True
            self.best_loss = current_loss if current_loss is not None else float("inf")
            self.last_best = self.best_loss
        eta, take_best, restart = self.eta, False, False
        if current_loss is not None:
            if current_loss < self.best_loss:
                self.best_loss = current_loss
                take_best = True
            if current_loss < self.last_best:
                self.count += 1
            if (i + 1) % self.INTERVAL == 0:
                if self.count / self.INTERVAL < self.RHO or self.best_loss == self.last_best:
                    self.eta /= 2
                    restart = True
                self.count = 0
                self.last_best = self.best_loss
        self.last = (eta, take_best, restart)
        return self.last

    def step(self, x: torch.Tensor, g: torch.Tensor, x0: torch.Tensor, current_loss: Optional[float], i: int,
             scratch: Optional[ops.L2Scratch] = None) -> torch.Tensor:
        """One call of the rule: a fresh output tensor (never `prev` or `best` themselves).  `scratch`: the run's ("l2")."""
        if self.prev is None:
            self.prev, self.best = x.clone(), x.clone()
        eta, take_best, restart = self.decide(current_loss, i)
        if self.norm == "l2":
            return ops.apgd_l2_step(x, g, x0, self.prev, self.best, self.eps, eta, take_best, restart, scratch=scratch)
        return ops.apgd_step(x, g, x0, self.prev, self.best, self.eps, eta, take_best, restart)

    def adopt(self, image: torch.Tensor) -> None:
        """Several ranks: rank 0's copy of the image returned by the latest call has overwritten this rank's -- take the
        state that call derived from its own output (best, and prev after a restart) from the synced pixels instead."""
        if self.last is None:
            return
        _, take_best, restart = self.last
        with torch.no_grad():
            if take_best:
                self.best.copy_(image.detach())
            if restart:
                self.prev.copy_(image.detach())


class ImageUpdate:
    """One run's image update (EngineOptions.pgd_rule, pgd_norm) and its state: the ApgdState of rule "apgd", and for norm
    "l2" the one L2Scratch (workspace + the last step's norms), allocated at the first step."""

    def __init__(self, rule: str, norm: str, eps: float, alpha: float):
        self.rule, self.norm, self.eps, self.alpha = rule, norm, eps, alpha
        self.apgd = ApgdState(eps, norm) if rule == "apgd" else None      # fresh per run, as the reference (:1337)
        self.scratch: Optional[ops.L2Scratch] = None
        self.n_steps = 0
        self._record: dict = {}

    def step(self, image: torch.Tensor, grad: torch.Tensor, x0: torch.Tensor, current_loss: Optional[float], i: int,
             record: bool = False) -> torch.Tensor:
        """The new image (requires grad) from the step's image, its gradient and the original image.  `current_loss`, `i`:
        the reference's arguments of the same names (auto-PGD only).  `record`: keep host copies for `stage_record`."""
        x = image.detach()
        if x.dtype != torch.float32:
            raise TypeError("the PGD image must be float32 (the reference feeds ToTensor() output)")
        x, g, x0 = x.contiguous(), grad.to(torch.float32).contiguous(), x0.detach().contiguous()
        a, l2 = self.apgd, self.norm == "l2"
        if l2 and self.scratch is None:
            self.scratch = ops.L2Scratch(x.device, x.numel())
        rec = {}
        if record and (a is not None or l2):
            rec = dict(x=x.cpu().numpy(), g=g.cpu().numpy())
            if a is not None:
                rec.update(prev_in=rec["x"] if a.prev is None else a.prev.cpu().numpy(),
                           best_in=rec["x"] if a.best is None else a.best.cpu().numpy())
        if a is not None:
            out = a.step(x, g, x0, current_loss, i, scratch=self.scratch)
        elif l2:
            out = ops.l2_step(x, g, x0, self.eps, self.alpha, scratch=self.scratch)
        else:
            out = ops.linf_step(x, g, x0, self.eps, self.alpha)
        if rec:
            if a is not None:
                eta, take_best, restart = a.last
                rec.update(current_loss=current_loss, eta=eta, take_best=take_best, restart=restart, eta_next=a.eta,
                           count=a.count, best_loss=a.best_loss, last_best=a.last_best, prev_out=a.prev.cpu().numpy(),
                           best_out=a.best.cpu().numpy())
                if l2:
                    rec.update(norm="l2")
            if l2:
                rec.update(out=out.cpu().numpy(), norms=self.scratch.norms.cpu().numpy())
            key = "apgd" if a is not None else "l2"
            rec = {key: rec}
            if self.n_steps == 0:
                rec[key + "_x0"] = x0.cpu().numpy()
        self._record = rec
        self.n_steps += 1
        return out.requires_grad_()

    def stage_record(self) -> dict:
        """What the latest `step(record=True)` adds to the step's trace entry: "l2" / "apgd" (inputs, outputs, flags and
        host state of the call) and, at the first step, "l2_x0" / "apgd_x0".  Nothing for the plain L-inf rule."""
        return self._record

    def adopt(self, image: torch.Tensor) -> None:
        """Several ranks: rank 0's image has overwritten this rank's; the state derived from the step's own output follows."""
        if self.apgd is not None:
            self.apgd.adopt(image)
