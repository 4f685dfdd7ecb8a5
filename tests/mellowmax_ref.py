"""References of the mellowmax target loss (loss_rule="mellowmax"; contract in include/bma.h, a2b) for test_mellowmax.py
and test_mellowmax_gpu.py: the float64 restatement, the float32 restatement of the kernel's operation order, the torch
restatement of the reference's function (its fp32 error against float64 is what the kernel's tolerance is measured
from), and seeded inputs that are exact in float32, bfloat16 and float16 alike."""

import math

import numpy as np
import torch

ALPHAS = (0.25, 1.0, 4.0)
POOL_ROWS = 64


def torch_mellowmax(t: torch.Tensor, alpha: float) -> torch.Tensor:
    """The reference's utils.mellowmax (bimodalattack/utils.py:35-36) restated in torch, dim = -1."""
    return 1.0 / alpha * (torch.logsumexp(alpha * t, dim=-1) - torch.log(torch.tensor(t.shape[-1], dtype=t.dtype)))


def gather_t(logits: np.ndarray, labels: np.ndarray) -> np.ndarray:
    """t[b, j] = -logits[b, j, labels[j]]."""
    return -logits[:, np.arange(labels.size), labels]


def restated64(t: np.ndarray, alpha: float):
    """(loss (B,), w (B, T)) in float64 by the contract: the maximum (NaN skipped; +-inf replaced by 0, torch.logsumexp's
    rule) out of the exponentials, w = exp(a - m) / s."""
    a = float(alpha) * np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        m = np.fmax.reduce(a, axis=-1, keepdims=True, initial=-np.inf)
        m = np.where(np.isinf(m), 0.0, m)
        e = np.exp(a - m)
        s = e.sum(-1, keepdims=True)
        loss = ((np.log(s) + m)[..., 0] - math.log(t.shape[-1])) / float(alpha)
        return loss, e / s


def autograd64(t: np.ndarray, alpha: float):
    """(loss, d loss / d t) of the torch restatement in float64 by torch autograd: what w must equal, special values
    (NaN patterns) included."""
    x = torch.from_numpy(np.asarray(t, np.float64)).requires_grad_()
    loss = torch_mellowmax(x, alpha)
    (g,) = torch.autograd.grad(loss.sum(), x)
    return loss.detach().numpy(), g.numpy()


def restated32_kernel_order(t: np.ndarray, alpha: float):
    """The kernel's own order in float32 (csrc/mellowmax_target.hip): n = 64 lanes (T <= 64) or 256; lane l folds rows
    l, l + n, ... in that order; the lanes of a wave are merged by an xor butterfly (32, 16, ... 1), the four waves in wave
    order.  numpy's float32 exp / log stand in for the device's."""
    f32 = np.float32
    t = np.asarray(t, f32)
    B, T = t.shape
    n = 64 if T <= 64 else 256
    loss, w = np.empty(B, f32), np.empty((B, T), f32)
    with np.errstate(all="ignore"):
        for b in range(B):
            a = f32(alpha) * t[b]
            m = f32(np.fmax.reduce(a, initial=f32(-np.inf)))
            if np.isinf(m):
                m = f32(0)
            e = np.exp(a - m).astype(f32)
            part = np.zeros(n, f32)
            for lane in range(min(n, T)):
                acc = f32(0)
                for j in range(lane, T, n):
                    acc = f32(acc + e[j]) if j != lane else e[j]
                part[lane] = acc
            part = part.reshape(-1, 64)
            idx = np.arange(64)
            for o in (32, 16, 8, 4, 2, 1):
                part = (part + part[:, idx ^ o]).astype(f32)
            s = part[0, 0]
            for wv in range(1, part.shape[0]):
                s = f32(s + part[wv, 0])
            loss[b] = f32(f32(f32(np.log(s)) + m) - f32(np.log(f32(T)))) / f32(alpha)
            w[b] = e / s
    return loss, w


def pool(T: int, rows: int = POOL_ROWS) -> np.ndarray:
    """`rows` seeded vectors of T target terms t = -logit: eighths in [-16, 16), exact in float32, bfloat16 and float16.
    The same pool serves every test of a T, so the reference and the bound are computed once per (T, alpha)."""
    rs = np.random.RandomState(1000 + T)
    return (rs.randint(-128, 128, size=(rows, T)) / 8.0).astype(np.float32)


_BOUNDS = {}


def bounds(t: np.ndarray, alpha: float, key=None):
    """(loss bound, w bound) of one (T, alpha) class: 4 x the largest error of the FP32 torch evaluation of the reference's
    function (and of its autograd) against float64 on the finite rows of `t`.  The factor covers the device's 1-ulp exp /
    log and the different summation order; nothing here comes from the kernel."""
    if key is not None and key in _BOUNDS:
        return _BOUNDS[key]
    t = np.asarray(t, np.float32)
    l64, g64 = autograd64(t, alpha)
    x = torch.from_numpy(t).requires_grad_()
    l32 = torch_mellowmax(x, alpha)
    ok = np.isfinite(l64) & np.isfinite(g64).all(-1)
    (g32,) = torch.autograd.grad(l32[torch.from_numpy(ok)].sum(), x)
    with np.errstate(invalid="ignore"):                      # (the special rows, masked out right away)
        el = np.abs(l32.detach().numpy().astype(np.float64) - l64)[ok]
        eg = np.abs(g32.numpy().astype(np.float64) - g64)[ok]
    out = (4.0 * float(el.max(initial=0.0)), 4.0 * float(eg.max(initial=0.0)))
    if key is not None:
        _BOUNDS[key] = out
    return out


def ulp(x: np.ndarray, dtype: torch.dtype) -> np.ndarray:
    """One rounding of `dtype` at |x| (half a unit in the last place, subnormal spacing below the smallest normal)."""
    bits = {torch.float32: (24, -126), torch.bfloat16: (8, -126), torch.float16: (11, -14)}[dtype]
    ax = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** bits[1])
    return 0.5 * 2.0 ** (np.floor(np.log2(ax)) - (bits[0] - 1))


def same_special(got: np.ndarray, want: np.ndarray) -> bool:
    """Non-finite entries agree exactly: NaN where NaN, the same infinity."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bad = ~np.isfinite(want)
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[bad & ~np.isnan(want)], want[bad & ~np.isnan(want)])
                and np.isfinite(got[~bad]).all())


# ---------------------------------------------------------------------------------------------------------------- whole runs
GOAL, TARGET = "tell me a story about cats", "Sure here is a story"
RUN_ALPHA = 0.5
MODES = {
    "gcg": dict(search_width=24, topk=32, pgd_attack=False, gcg_attack=True),
    "pgd": dict(pgd_attack=True, gcg_attack=False, eps=64 / 255, alpha=4 / 255),
    "joint": dict(search_width=24, topk=32, pgd_attack=True, gcg_attack=True, joint_eval=True, eps=64 / 255, alpha=4 / 255),
}
CASES = [("llava", "gcg"), ("llava", "pgd"), ("llava", "joint"), ("gemma3", "gcg"), ("gemma3", "pgd"), ("gemma3", "joint")]
EARLY = dict(kind="llava", mode="gcg", target=";", steps=8)       # the early-stop run of both test files


def messages_for(kind: str, mode: str):
    """What run() is given as `messages`.  Gemma-3's template walks `content` as a list of items, so its GCG-only prompt
    (no image item) is given in list form, with the suffix slot in the text item; every other case is the plain string."""
    if kind == "gemma3" and mode == "gcg":
        return [{"role": "user", "content": [{"type": "text", "text": GOAL + " {optim_str}"}]}]
    return GOAL


def run_config(mode: str, steps: int = 4, **over):
    import tempfile
    from bimodalattack_amd import GCGConfig, synthetic as S
    return GCGConfig(seed=1, verbosity="ERROR", optim_str_init=S.TINY_OPTIM_INIT, images_folder=tempfile.mkdtemp(prefix="bma_mm_"),
                     **{**MODES[mode], "num_steps": steps, "use_mellowmax": True, "mellowmax_alpha": RUN_ALPHA, **over})


def loss_tol(scale: float) -> float:
    """The loss moves by no more than the T target logits do (its weights are a convex combination).  The engine's fp32
    forward of the tiny models and the plain HF forward on the CPU agree to a few 1e-6 of the logits' magnitude (the default
    rule's trajectories hold the cross-entropy, a difference of such logits, to rtol 1e-4 of values around 5)."""
    return 1e-4 * max(1.0, scale)


def reference_run(kind: str, mode: str, steps: int = 4, target: str = TARGET, **over):
    """The whole attack on the CPU under the mellowmax rule: the oracle's loop (prompt, sampling, filter, PGD step, order
    of random draws) with its two loss sites replaced by the float64 rule on the plain fp32 HF forward.  Returns (result
    dict, trace); each trace step also has "near_tie" (top two candidate losses within loss_tol) and "hit"."""
    from bimodalattack_amd import synthetic as S
    from oracle.attack_loop import OracleAttack

    class MellowOracle(OracleAttack):
        def _mm(self, rows):
            T = self.target_ids.shape[1]
            return torch_mellowmax(-rows.double()[:, torch.arange(T), self.target_ids[0]], RUN_ALPHA)

        def _score(self, chunk, embeds):
            T = self.target_ids.shape[1]
            with torch.no_grad():
                rows = self.model(inputs_embeds=embeds).logits[:, embeds.shape[1] - T - 1:-1, :]
            hit = (rows.argmax(-1) == self.target_ids[0]).all(-1)
            if self.cfg.early_stop and bool(hit.any()):
                self.stop = True
            loss = self._mm(rows)
            if embeds.shape[0] > 1:
                two = np.sort(loss.numpy())[:2]
                scale = float(rows[:, torch.arange(T), self.target_ids[0]].abs().max())
                self.notes.append(dict(near_tie=bool(two[1] - two[0] <= loss_tol(scale)), hit=bool(hit.any())))
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
            loss = self._mm(self.model(inputs_embeds=x).logits[:, x.shape[1] - T - 1:-1, :])[0]
            wanted = ([onehot] if cfg.gcg_attack else []) + ([image] if cfg.pgd_attack else [])
            grads = list(torch.autograd.grad(loss, wanted))
            return (grads.pop(0) if cfg.gcg_attack else None), (grads.pop(0) if cfg.pgd_attack else None)

    model, tok, proc, image = S.tiny_case(kind, device="cpu")
    cfg = run_config(mode, steps, **over)
    atk = MellowOracle(model, tok, proc, cfg, S.Normalize(S.CLIP_MEAN, S.CLIP_STD))
    atk.notes = []
    res = atk.run(messages_for(kind, mode), GOAL, target, image if cfg.pgd_attack else None)
    return res, atk.trace, atk.notes
