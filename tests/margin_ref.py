"""References of the Carlini-Wagner margin target loss (loss_rule="margin"; contract in include/bma.h, a2c) for
test_margin.py and test_margin_gpu.py: the float64 restatement of the contract, the torch restatement (masked max,
subtract, clamp, mean), seeded inputs that are exact in float32, bfloat16 and float16 alike (and full of tied maxima), a
generic pool for the rounding bound, and the whole attack on the CPU under the rule.  No kernel is touched here."""

import numpy as np
import torch

from mellowmax_ref import CASES, EARLY, GOAL, MODES, TARGET, loss_tol, messages_for   # shared by the whole-run tests

RUN_KAPPA = 0.05


# ------------------------------------------------------------------------------------------------- the rule, restated
def restated64(z, labels, kappa, grad_scale=1.0, exclude_label=True, tie="first", strict=False):
    """The contract in float64 on (B, T, V) logits that are already rounded to their dtype.  Returns a dict: loss (B,),
    m (B, T), i (B, T) int (-1: every v != y is NaN), a (B, T) bool, match (B,) bool, dlogits (B, T, V) holding 0 and
    -+g with g = float32(grad_scale) / float32(T), the value the kernel rounds to the dtype.

    exclude_label / tie / strict select the three mutants the tests tell apart from the rule: the label left in the
    maximum, the LAST index among tied maxima, and a strict `>` in a_j."""
    z = np.asarray(z, np.float64)
    labels = np.asarray(labels, np.int64)
    B, T, V = z.shape
    rows = np.arange(T)
    valid = (labels >= 0) & (labels < V)
    lab = np.where(valid, labels, 0)
    nan = np.isnan(z)

    def first_max(cand, last=False):
        """(value, index) of the first (mutant: last) maximum among the elements `cand` allows; (-inf, -1) where it
        allows none."""
        top = np.where(cand, z, -np.inf).max(-1)
        eq = cand & (z == top[..., None])
        idx = V - 1 - eq[..., ::-1].argmax(-1) if last else eq.argmax(-1)
        idx = np.where(eq.any(-1), idx, -1)
        val = np.take_along_axis(z, np.maximum(idx, 0)[..., None], -1)[..., 0]      # z[i]: keeps the sign of a zero
        return np.where(idx >= 0, val, -np.inf), idx

    excl = np.zeros((T, V), bool)
    if exclude_label:
        excl[rows[valid], lab[valid]] = True
    o, i = first_max(~nan & ~excl[None], last=tie != "first")
    zl = z[:, rows, lab]
    bad = nan.any(-1) | ~valid[None]
    with np.errstate(invalid="ignore"):
        m = np.where(bad, np.nan, o - zl)
        l = np.where(m < -kappa, -kappa, m)                                         # NaN stays
        loss = l.sum(-1) / T
        a = (m > -kappa) if strict else (m >= -kappa)
    _, top1 = first_max(~nan)                                                       # (the tie mutant changes i only)
    match = (valid[None] & (top1 == labels[None])).all(-1)
    g = float(np.float32(grad_scale) / np.float32(T))
    d = np.zeros((B, T, V), np.float64)
    bb, jj = np.nonzero(a)
    d[bb, jj, lab[jj]] = -g
    d[bb, jj, i[bb, jj]] = g
    return dict(loss=loss, m=m, i=i, a=a, match=match, dlogits=d)


def torch_margin(z: torch.Tensor, labels: torch.Tensor, kappa: float) -> torch.Tensor:
    """The rule in torch on (..., T, V): masked max, subtract, clamp, mean.  Which of several tied maxima torch.max's
    backward feeds is torch's business: compare gradients on rows without ties only."""
    onehot = torch.nn.functional.one_hot(labels, z.shape[-1]).bool()
    o = z.masked_fill(onehot, float("-inf")).max(-1).values
    m = o - z.gather(-1, labels.expand(z.shape[:-1]).unsqueeze(-1)).squeeze(-1)
    return m.clamp(min=-kappa).mean(-1)


def autograd64(z, labels, kappa, grad_scale=1.0):
    """(loss (B,), d (grad_scale * sum_b loss_b) / d z) of the torch restatement in float64."""
    x = torch.from_numpy(np.asarray(z, np.float64)).requires_grad_()
    loss = torch_margin(x, torch.from_numpy(np.asarray(labels, np.int64)), kappa)
    (g,) = torch.autograd.grad(grad_scale * loss.sum(), x)
    return loss.detach().numpy(), g.numpy()


# ------------------------------------------------------------------------------------------------------------- inputs
def grid_pool(B: int, T: int, V: int, seed: int = 0) -> np.ndarray:
    """(B, T, V) eighths in [-16, 16): exact in float32, bfloat16 and float16, 256 distinct values -- tied maxima in
    every row once V passes a few hundred.  Margins and their sums are exact in float32, so the expected loss is
    float32(float64 sum / T), bit for bit."""
    rs = np.random.RandomState(2000 + seed + 31 * T + V)
    return (rs.randint(-128, 128, size=(B, T, V)) / 8.0).astype(np.float32)


def generic_pool(B: int, T: int, V: int, seed: int = 0) -> np.ndarray:
    """(B, T, V) generic float32 values (normal, sigma 4): margins that round, for the loss's rounding bound."""
    rs = np.random.RandomState(3000 + seed + 31 * T + V)
    return (4.0 * rs.standard_normal(size=(B, T, V))).astype(np.float32)


def labels_for(T: int, V: int, seed: int = 0) -> np.ndarray:
    lab = np.random.RandomState(seed + 7 * T + V).randint(0, V, size=T).astype(np.int64)
    lab[0], lab[-1] = 0, V - 1                                   # (T = 1: V - 1)
    return lab


def expected_loss32(ref) -> np.ndarray:
    """The loss the kernel must return bit for bit on the grid pool."""
    return ref["loss"].astype(np.float32)


def loss_bound(ref, T: int, kappa: float) -> np.ndarray:
    """Generic inputs: one rounding per row subtraction, T - 1 in the sum, one in the division -- (T + 2) roundings of
    2^-24 relative to the mean |l_j| (every partial sum is bounded by the sum of the |l_j|)."""
    with np.errstate(invalid="ignore"):
        l = np.where(ref["m"] < -kappa, -kappa, ref["m"])
    return (T + 2) * 2.0 ** -24 * np.abs(l).mean(-1)


# ---------------------------------------------------------------------------------------------------------- whole runs
def run_config(mode: str, steps: int = 4, **over):
    import tempfile
    from bimodalattack_amd import GCGConfig, synthetic as S
    return GCGConfig(seed=1, verbosity="ERROR", optim_str_init=S.TINY_OPTIM_INIT, images_folder=tempfile.mkdtemp(prefix="bma_mg_"),
                     **{**MODES[mode], "num_steps": steps, **over})


def row_facts(rows: torch.Tensor, labels: torch.Tensor, kappa: float):
    """Of (B, T, V) target rows in float64: the margins m (B, T), the gap between the two best non-label logits (B, T),
    and the largest |logit| among the label and runner-up logits."""
    rows = rows.double()
    onehot = torch.nn.functional.one_hot(labels, rows.shape[-1]).bool()
    top2 = rows.masked_fill(onehot, float("-inf")).topk(2, dim=-1).values
    zl = rows.gather(-1, labels.expand(rows.shape[:-1]).unsqueeze(-1)).squeeze(-1)
    scale = float(torch.maximum(zl.abs().max(), top2[..., 0].abs().max()))
    return top2[..., 0] - zl, top2[..., 0] - top2[..., 1], scale


def reference_run(kind: str, mode: str, steps: int = 4, target: str = TARGET, kappa: float = RUN_KAPPA, **over):
    """The whole attack on the CPU under the margin rule: the oracle's loop (prompt, sampling, filter, PGD step, order of
    random draws) with its two loss sites replaced by the float64 rule on the plain fp32 HF forward.  Returns (result
    dict, trace, notes, grad_notes).  notes, one per scoring step with candidates: near_tie (the two best candidate
    losses within loss_tol), hit, clamped (the winner has a row below -kappa), gap.  grad_notes, one per gradient site:
    fragile (some row has its two best non-label logits within loss_tol, or |m_j + kappa| within it: the gradient is
    discontinuous there), gap."""
    from bimodalattack_amd import synthetic as S
    from oracle.attack_loop import OracleAttack

    class MarginOracle(OracleAttack):
        def _rule(self, rows):
            return torch_margin(rows.double(), self.target_ids[0], kappa)

        def _score(self, chunk, embeds):
            T = self.target_ids.shape[1]
            with torch.no_grad():
                rows = self.model(inputs_embeds=embeds).logits[:, embeds.shape[1] - T - 1:-1, :]
            hit = (rows.argmax(-1) == self.target_ids[0]).all(-1)
            if self.cfg.early_stop and bool(hit.any()):
                self.stop = True
            loss = self._rule(rows)
            if embeds.shape[0] > 1:
                m, _, scale = row_facts(rows, self.target_ids[0], kappa)
                two = np.sort(loss.numpy())[:2]
                self.notes.append(dict(near_tie=bool(two[1] - two[0] <= loss_tol(scale)), hit=bool(hit.any()),
                                       clamped=bool((m[int(loss.argmin())] < -kappa).any()), gap=float(two[1] - two[0])))
            return loss.to(rows.dtype)

        def _gradient(self, optim_ids, image=None):
            cfg = self.cfg
            V = self.emb.num_embeddings
            onehot = torch.nn.functional.one_hot(optim_ids, num_classes=V).to(self.model.dtype)
            if cfg.gcg_attack:
                onehot.requires_grad_()
            optim = onehot @ self.emb.weight
            if cfg.pgd_attack:
                parts = [self.seg["before_img"], self._image_features(image), self.seg["before_suffix"], optim,
                         self.seg["after"], self.seg["target"]]
            else:
                parts = [self.seg["before"], optim, self.seg["after"], self.seg["target"]]
            x = torch.cat(parts, dim=1)
            T = self.target_ids.shape[1]
            rows = self.model(inputs_embeds=x).logits[:, x.shape[1] - T - 1:-1, :]
            m, gap, scale = row_facts(rows.detach(), self.target_ids[0], kappa)
            tol = loss_tol(scale)
            self.grad_notes.append(dict(fragile=bool((gap <= tol).any() or ((m + kappa).abs() <= tol).any()),
                                        gap=float(torch.minimum(gap.min(), (m + kappa).abs().min())), tol=tol))
            loss = self._rule(rows)[0]
            wanted = ([onehot] if cfg.gcg_attack else []) + ([image] if cfg.pgd_attack else [])
            grads = list(torch.autograd.grad(loss, wanted))
            return (grads.pop(0) if cfg.gcg_attack else None), (grads.pop(0) if cfg.pgd_attack else None)

    model, tok, proc, image = S.tiny_case(kind, device="cpu")
    cfg = run_config(mode, steps, **over)
    atk = MarginOracle(model, tok, proc, cfg, S.Normalize(S.CLIP_MEAN, S.CLIP_STD))
    atk.notes, atk.grad_notes = [], []
    res = atk.run(messages_for(kind, mode), GOAL, target, image if cfg.pgd_attack else None)
    return res, atk.trace, atk.notes, atk.grad_notes
