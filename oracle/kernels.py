"""ORACLE -- test infrastructure, not product code.

CPU restatement (numpy) of the small per-step pieces of the reference's hot
path.  Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s
``cpu_baseline`` leg may import this package; the product
(``bimodalattack_amd``) never does and fails loudly without its HIP library.

Parity status: PINNED.  Every function here is checked against golden vectors
captured from the real reference (``tests/golden/make_golden.py`` ->
``tests/golden/g1..g6``) by ``tests/test_oracle_golden.py``; the auto-PGD restatement against ``g8_apgd_unit``
by ``tests/test_apgd.py``.  The L2 restatements have no reference: ``tests/test_pgd_l2.py`` holds them to the contract.

Citations are into /root/reference/bimodalattack/bimodal_attack.py unless a
file is named.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch


# --------------------------------------------------------------------------
# a5 -- PGD L-inf step (reference :1030-1037)
# --------------------------------------------------------------------------
def linf_step(x: np.ndarray, g: np.ndarray, x0: np.ndarray, eps: float, alpha: float) -> np.ndarray:
    """x' = clamp(clamp(x - (alpha*eps)*sign(g), x0-eps, x0+eps), 0, 1) in fp32.

    The reference's step is alpha*eps (a Python double product, :1033) applied
    as an fp32 scalar; the ball radius is eps as an fp32 scalar (:1034)."""
    x = np.asarray(x, np.float32)
    g = np.asarray(g, np.float32)
    x0 = np.asarray(x0, np.float32)
    step = np.float32(alpha * eps)
    e = np.float32(eps)
    sgn = (g > 0).astype(np.float32) - (g < 0).astype(np.float32)   # torch.sign: 0 for NaN and for -0.0
    y = (x - step * sgn).astype(np.float32)
    lo = (x0 - e).astype(np.float32)
    hi = (x0 + e).astype(np.float32)
    y = np.where(y < lo, lo, y)
    y = np.where(y > hi, hi, y)
    y = np.where(y < np.float32(0), np.float32(0), y)
    y = np.where(y > np.float32(1), np.float32(1), y)
    return y.astype(np.float32)


# --------------------------------------------------------------------------
# a5b -- auto-PGD L-inf step (reference :1039-1110), the per-pixel part of one call
# --------------------------------------------------------------------------
def _tmin(a, b):
    """torch.min(a, b): NaN from either operand, the first operand on a tie."""
    r = np.where(b < a, b, a)
    return np.where(np.isnan(a), a, np.where(np.isnan(b), b, r))


def _tmax(a, b):
    r = np.where(a < b, b, a)
    return np.where(np.isnan(a), a, np.where(np.isnan(b), b, r))


def _clamp01(y):
    y = np.where(y < 0, np.float32(0), y)
    return np.where(y > 1, np.float32(1), y)


def apgd_restated(x, g, x0, prev, best, eps, eta, take_best, restart):
    """One call of the rule's per-pixel part, each operation rounded in float32 as the reference's torch ops round it.
    Returns (out, prev, best) after the call."""
    x, g, x0, prev, best = (np.asarray(a, np.float32) for a in (x, g, x0, prev, best))
    if restart and not take_best:
        return best.copy(), best.copy(), best.copy()
    with np.errstate(invalid="ignore"):
        s = (g > 0).astype(np.float32) - (g < 0).astype(np.float32)
        hi, lo = x0 + np.float32(eps), x0 - np.float32(eps)
        z = _clamp01(_tmax(_tmin(x - np.float32(eta) * s, hi), lo))
        m = (x + np.float32(0.75) * (z - x)) + np.float32(0.25) * (x - prev)
        new = _clamp01(_tmax(_tmin(m, hi), lo))
    return new, (new if restart else x).copy(), (new if take_best else best).copy()


def same_bits(a, b) -> bool:
    """Equal bit for bit, any NaN equal to any NaN (torch's scalar and vector paths write different NaN payloads)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))


# --------------------------------------------------------------------------
# a5c -- both rules in the L2 ball (no reference: the contract of include/bma.h, restated in torch fp32 ops)
# --------------------------------------------------------------------------
ULP = 2.0 ** -24          # one fp32 rounding, relative


def as_f32(a):
    return torch.as_tensor(np.asarray(a, np.float32))


def f32_scalar(v):
    """A Python float rounded to fp32 the way the C ABI's `float` parameter rounds it."""
    return torch.tensor(float(v), dtype=torch.float32)


def _nrm(v):
    """nrm(v) = float32(sqrt(sum double(v_i)^2)): fp64 accumulation, rounded once."""
    return v.double().pow(2).sum().sqrt().to(torch.float32)


def l2_clamp01(y):
    """compare+select: keeps -0.0, propagates NaN."""
    y = torch.where(y < 0, torch.zeros((), dtype=torch.float32), y)
    return torch.where(y > 1, torch.ones((), dtype=torch.float32), y)


def _project(y, x0, eps):
    """(clamp01(x0 + (y - x0) * f), nrm(y - x0)),  f = minimum(eps / nrm, 1): a zero norm gives inf and f = 1."""
    d = y - x0
    nd = _nrm(d)
    f = torch.minimum(eps / nd, torch.ones((), dtype=torch.float32))
    return l2_clamp01(x0 + d * f), nd


def l2_descent(x, g, step):
    ng = _nrm(g)
    u = g / (ng + f32_scalar(1e-10))
    return x - step * u, ng             # multiply, then subtract


def l2_restated(x, g, x0, eps, step):
    """One plain L2 step, fp32 operation by operation in the order of the contract.  Returns (out, norms[2]) as numpy."""
    x, g, x0 = as_f32(x), as_f32(g), as_f32(x0)
    y, ng = l2_descent(x, g, f32_scalar(step))
    out, nd = _project(y, x0, f32_scalar(eps))
    return out.numpy(), np.array([ng.item(), nd.item()], np.float32)


def apgd_l2_restated(x, g, x0, prev, best, eps, eta, take_best, restart):
    """One auto-PGD call in the L2 ball.  Returns (out, prev, best, norms[3]) after the call; norms is None on the
    "restart without take_best" shortcut, which reads only `best` and leaves the norms alone."""
    x, g, x0, prev, best = (as_f32(a) for a in (x, g, x0, prev, best))
    if restart and not take_best:
        b = best.numpy()
        return b.copy(), b.copy(), b.copy(), None
    y, ng = l2_descent(x, g, f32_scalar(eta))
    z, nd = _project(y, x0, f32_scalar(eps))
    m = (x + f32_scalar(0.75) * (z - x)) + f32_scalar(0.25) * (x - prev)
    new, nm = _project(m, x0, f32_scalar(eps))
    new = new.numpy()
    return (new, (new if restart else x.numpy()).copy(), (new if take_best else best.numpy()).copy(),
            np.array([ng.item(), nd.item(), nm.item()], np.float32))


def dist64(a, b):
    return float(np.sqrt(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).sum()))


# --------------------------------------------------------------------------
# a2 -- cross-entropy over the target slice (reference :1006-1012, :1289-1298)
# --------------------------------------------------------------------------
def ce_rows(logits: np.ndarray, labels: np.ndarray) -> np.ndarray:
    """Per-row CE of logits (..., T, V) against labels (T,): logsumexp - x[label].
    Accumulates in float64: this is the 'truth' both the reference's fp32 result
    and the kernel's fp32 result are compared to."""
    x = np.asarray(logits, np.float64)
    m = x.max(axis=-1, keepdims=True)
    lse = np.log(np.exp(x - m).sum(axis=-1)) + m[..., 0]
    lab = np.asarray(labels, np.int64).reshape(-1)
    picked = np.take_along_axis(x, np.broadcast_to(lab.reshape((1,) * (x.ndim - 2) + (-1, 1)), x.shape[:-1] + (1,)), axis=-1)[..., 0]
    return lse - picked


def ce_target(logits: np.ndarray, labels: np.ndarray):
    """Candidate scoring (:1289-1306): logits (B,T,V), labels (T,) ->
    (loss (B,) = mean over T, match (B,) = every row's argmax equals its label)."""
    rows = ce_rows(logits, labels)
    lab = np.asarray(labels, np.int64).reshape(-1)
    match = (np.argmax(np.asarray(logits), axis=-1) == lab[None, :]).all(axis=-1)
    return rows.mean(axis=-1), match


def ce_target_grad(logits: np.ndarray, labels: np.ndarray, scale: float = 1.0) -> np.ndarray:
    """d(mean CE)/d(logits) for one sequence (T,V): (softmax - onehot) / T * scale
    (what autograd hands back through :1010-1012)."""
    x = np.asarray(logits, np.float64)
    T = x.shape[-2]
    m = x.max(axis=-1, keepdims=True)
    p = np.exp(x - m)
    p /= p.sum(axis=-1, keepdims=True)
    lab = np.asarray(labels, np.int64).reshape(-1)
    p[np.arange(T), lab] -= 1.0
    return p * (scale / T)


# --------------------------------------------------------------------------
# a3 -- candidate sampling (reference :130-163)
# --------------------------------------------------------------------------
def mask_topk(grad: np.ndarray, not_allowed: Optional[np.ndarray], k: int) -> np.ndarray:
    """Per position, the k token ids with the most negative gradient among the
    allowed ones (:144-147): not-allowed columns count as +inf.  Order: gradient
    ascending, ties by lower token id (the build's tie policy; the reference's
    own goldens are tie-free).  NaN gradients rank first, as torch.topk(-grad)
    ranks NaN above everything."""
    g = np.array(grad, dtype=np.float32, copy=True)
    if not_allowed is not None and len(not_allowed):
        g[:, np.asarray(not_allowed, np.int64)] = np.inf
    g = np.where(np.isnan(g), -np.inf, g)
    order = np.argsort(g, axis=1, kind="stable")
    return order[:, :k].astype(np.int64)


def rand_positions(rnd: np.ndarray, n_replace: int) -> np.ndarray:
    """argsort(rand)[..., :n_replace] (:150-154): the n_replace positions with the
    smallest random keys, in that order."""
    return np.argsort(np.asarray(rnd), axis=1, kind="stable")[:, :n_replace].astype(np.int64)


def sample_scatter(ids: np.ndarray, topk_idx: np.ndarray, pos: np.ndarray, rank: np.ndarray) -> np.ndarray:
    """new_ids[b] = ids with position pos[b,j] replaced by topk_idx[pos[b,j], rank[b,j]]
    (:142, :156-162)."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    B, n_rep = pos.shape
    out = np.tile(ids, (B, 1))
    for j in range(n_rep):
        out[np.arange(B), pos[:, j]] = topk_idx[pos[:, j], rank[:, j]]
    return out


def sample_ids_from_grad(ids, grad, topk: int, n_replace: int, not_allowed, rnd, rank) -> np.ndarray:
    """The whole of :130-163 with the two random draws passed in as inputs
    (rnd: (sw, n_opt) uniform floats; rank: (sw, n_replace) ints in [0, topk))."""
    tk = mask_topk(grad, not_allowed, topk)
    pos = rand_positions(rnd, n_replace)
    return sample_scatter(ids, tk, pos, np.asarray(rank, np.int64))


def dynamic_width(step: int, search_width: int, num_steps: int, min_search_width: int, dynamic: bool) -> int:
    """:919-928."""
    if not dynamic:
        return search_width
    return max(min_search_width, int(search_width * (1 - step / num_steps)))


# --------------------------------------------------------------------------
# a7 -- embedding splice (reference :1112-1225)
# --------------------------------------------------------------------------
def segment_order(mode: str, model_type: str, single: bool = False, no_joint_eval: bool = False,
                  no_target: bool = False) -> List[str]:
    """Which segments, in which order (:1150-1215).  ``gemma3`` puts the suffix in
    front of the image; everything else puts it behind."""
    g = model_type == "gemma3"
    with_img = (["before_img", "optim", "before_suffix", "image", "after"] if g
                else ["before_img", "image", "before_suffix", "optim", "after"])
    if mode == "pgd":
        if not single:
            raise AssertionError("PGD mode only supports single=True")
        return with_img + ["target"]
    if mode == "gcg":
        if single:
            return (["before_img", "optim", "before_suffix", "after", "target"] if g
                    else ["before_img", "before_suffix", "optim", "after", "target"])
        if no_joint_eval:
            return ["before", "optim", "after", "target"]
        if no_target:
            return ["before", "optim", "after"]
        raise ValueError("Invalid flags for BimodalAttack mode")
    if mode == "gcg_pgd":
        if not single and no_target:
            return with_img
        return with_img + ["target"]
    raise ValueError(f"Unknown mode '{mode}'")


def splice(order: Sequence[str], segments: Dict[str, np.ndarray], table: np.ndarray, ids: np.ndarray,
           search_width: Optional[int], emb_scale: Optional[float] = None) -> np.ndarray:
    """Concatenate segments along the sequence axis (:1217-1225).  'optim' is the
    embedding gather table[ids] (times the Gemma embedding scale when the model's
    embedding layer has one, :1142); every other segment is (1,L,D) and is
    repeated to ``search_width`` rows when search_width is given."""
    ids = np.asarray(ids, np.int64)
    parts = []
    for name in order:
        if name == "optim":
            t = table[ids]
            if emb_scale is not None:
                t = (t * table.dtype.type(emb_scale)).astype(table.dtype)
        else:
            t = segments[name]
        if search_width is not None and t.shape[0] == 1:
            t = np.repeat(t, search_width, axis=0)
        parts.append(t)
    return np.concatenate(parts, axis=1)


# --------------------------------------------------------------------------
# a4 / a9 -- tokenizer-side helpers
# --------------------------------------------------------------------------
def nonascii_tokens(tokenizer) -> np.ndarray:
    """reference utils.py:14-33: ids in range(vocab_size) whose decoded text is not
    printable ASCII, then bos/eos/pad/unk appended (duplicates kept)."""
    bad = [i for i in range(tokenizer.vocab_size)
           if not (lambda s: s.isascii() and s.isprintable())(tokenizer.decode([i]))]
    for attr in ("bos_token_id", "eos_token_id", "pad_token_id", "unk_token_id"):
        v = getattr(tokenizer, attr)
        if v is not None:
            bad.append(v)
    return np.asarray(bad, np.int64)


def filter_ids(ids: np.ndarray, tokenizer) -> np.ndarray:
    """:166-186, one string at a time: keep rows that decode -> encode back to
    themselves.  Raises RuntimeError when nothing survives."""
    ids = np.asarray(ids, np.int64)
    texts = tokenizer.batch_decode(ids.tolist())
    keep = []
    for row, text in zip(ids, texts):
        again = tokenizer(text, add_special_tokens=False)["input_ids"]
        if len(again) == len(row) and all(int(a) == int(b) for a, b in zip(again, row)):
            keep.append(row)
    if not keep:
        raise RuntimeError(
            "No token sequences are the same after decoding and re-encoding. "
            "Consider setting filter_ids=False or trying a different optim_str_init"
        )
    return np.stack(keep)
