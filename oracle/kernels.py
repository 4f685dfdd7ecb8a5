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


# --------------------------------------------------------------------------
# backward elementwise kernels (csrc/fused_elementwise.hip: rmsnorm_bwd_kernel, swiglu_bwd_kernel, rope with sin_sign = -1)
# --------------------------------------------------------------------------
# No reference program: the formulas in the comment block above rmsnorm_bwd_kernel, evaluated in float64 on operands
# already rounded to the model dtype, and the error bounds a correct fp32 evaluation of them keeps.  Written in torch
# float64 (not numpy) so that the largest case can stay on the device; numpy arrays are accepted.  Used by
# tests/test_backward_refs.py (CPU: the references against autograd, the bounds against a restatement of the kernels
# and against mutants of it) and tests/test_backward_gpu.py (the kernels).
from collections import namedtuple

# dtype -> (significand bits p, exponent of the smallest normal number)
_FORMATS = {torch.bfloat16: (8, -126), torch.float16: (11, -14), torch.float32: (24, -126)}
U32 = 2.0 ** -24                         # one fp32 rounding, relative
GELU_BETA, GELU_KAPPA = 0.7978845608028654, 0.044715   # sqrt(2/pi) and aten's kappa; the kernel rounds both to fp32
SILU_DZERO, GELU_DZERO = -1.2785, -0.7525            # zeros of silu' and of gelu-tanh'


def unit_roundoff(dt) -> float:
    """u: half the spacing of dtype `dt` relative to a value (2^-8 bf16, 2^-11 fp16, 2^-24 fp32)."""
    return 2.0 ** -_FORMATS[dt][0]


def half_subnormal(dt) -> float:
    """Half the subnormal spacing of `dt` (fp16: 2^-25): the absolute rounding error below the smallest normal."""
    p, emin = _FORMATS[dt]
    return 2.0 ** (emin - p)


def f64(a):
    return (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(torch.float64)


def round_dt(a, dt):
    """float64 -> the nearest value of `dt` (ties to even, gradual underflow, overflow to inf), as float64.  One
    rounding, done on the float64 bits: a conversion through fp32 would round twice."""
    a = f64(a)
    p, emin = _FORMATS[dt]
    e = ((a.view(torch.int64) >> 52) & 0x7FF) - 1023                  # floor(log2 |a|) of a normal double
    k = torch.clamp(e, min=emin) - (p - 1)                            # exponent of the spacing of dt at a
    q = ((k + 1023) << 52).view(torch.float64)
    r = torch.round(a / q) * q                                        # torch.round: halves to even
    top = (2.0 - 2.0 ** (1 - p)) * 2.0 ** (127 if dt != torch.float16 else 15)
    r = torch.where(r.abs() > top, torch.sign(a) * float("inf"), r)
    return torch.where(torch.isfinite(a), r, a)


NormBwdRef = namedtuple("NormBwdRef", "ref dxn rg xk")


def rmsnorm_bwd_ref(x, w, dy, eps, gemma, dsum=None) -> NormBwdRef:
    """dxn = r*g - x*k per row, g = dy*w (Llama) or dy*(1+w) (Gemma), r = 1/sqrt(mean(x^2)+eps), k = r^3*sum(g*x)/D, in
    float64 on operands (rows, D) already rounded to the model dtype; `eps` as the fp32 number the C entry point gets.
    ref = dxn, or dsum + dxn given the gradient of the residual stream.  rg = |r*g| and xk = |x|*r^3*sum|g*x|/D are
    the sizes of the two terms before they cancel, which is what an fp32 evaluation's error scales with."""
    x, w, dy = f64(x), f64(w), f64(dy)
    D = x.shape[-1]
    eps = float(np.float32(eps))
    g = dy * (1.0 + w if gemma else w)
    r = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    k = r ** 3 * (g * x).sum(-1, keepdim=True) / D
    dxn = r * g - x * k
    rg = (r * g).abs()
    xk = x.abs() * r ** 3 * (g * x).abs().sum(-1, keepdim=True) / D
    return NormBwdRef(dxn if dsum is None else f64(dsum) + dxn, dxn, rg, xk)


# The longest chain of fp32 roundings behind one output of rmsnorm_bwd_kernel: 32 sequential adds in a lane (4 chunks of
# 8), 6 levels of the wave reduction and 4 partials = 42 adds, the product under the sum and dy*(1+w) = 45; the division,
# square root and reciprocal of r = 3; r^3*tsg/D = 4; the two output products and the subtraction = 3.  55, rounded up
# to a power of two, each taken as one relative rounding of a quantity no larger than M = rg + xk.  The count is of the
# chain, not a worst case compounded through r^3: the roundings of a 42-term sum are independent and stay far below
# 42 half-units together (tests/test_backward_refs.py records how much of the bound a faithful evaluation uses).
NORM_BWD_C = 64


def norm_bwd_tol(ref: NormBwdRef, dt, with_dsum: bool):
    """Largest |got - ref.ref| a correct kernel leaves, per element: the one rounding to `dt` of the result, the fp32
    evaluation (NORM_BWD_C roundings of the uncancelled size), the rounding's subnormal floor -- and with `dsum` the
    rounding of dxn before the add, with its own floor."""
    u, fl = unit_roundoff(dt), half_subnormal(dt)
    tol = u * ref.ref.abs() + NORM_BWD_C * U32 * (ref.rg + ref.xk) + fl
    if with_dsum:
        tol = tol + u * ref.dxn.abs() + fl
    return tol


def gated_act_bwd_ref(gate, up, dy, act):
    """(act64(gate), act'64(gate), d_gate = dy*up*act'(gate)) in float64; act 0 = SiLU, 1 = GELU-tanh with the kernel's
    constants sqrt(2/pi) and 0.044715 (their rounding to fp32 is part of the kernel's error, counted below)."""
    g, up, dy = f64(gate), f64(up), f64(dy)
    if act == 0:
        s = torch.sigmoid(g)
        a, d = g * s, s * (1.0 + g * (1.0 - s))
    else:
        g2 = g * g
        t = torch.tanh(GELU_BETA * (g + GELU_KAPPA * g2 * g))
        a = 0.5 * g * (1.0 + t)
        d = 0.5 * (1.0 + t) + 0.5 * g * (1.0 - t * t) * GELU_BETA * (1.0 + 3.0 * GELU_KAPPA * g2)
    return a, d, dy * up * d


# swiglu_bwd_kernel's act'(g) in fp32, first-order worst case in units of 2^-24 * (1 + |g|*(1 + 3*kappa*g^2 [GELU])).
# Assumed accuracy of the device functions: expf within 3 ulp, tanhf within 5 ulp -- the OpenCL full-profile limits the
# ROCm device library is written to; the HIP math-API table (which lists smaller figures) is not part of a ROCm install.
#   SiLU, a = 3:  e = expf(-g): a.  1+e: a+1.  s = 1/(1+e): a+2 (relative, so at most a+2 absolute).  1-s: a+2.
#     g*(1-s): (a+3)|g|.  1+..: (a+3)|g| + (1+|g|).  s*(..): + (a+2)(1+|g|) + (1+|g|)  ->  (2a+7)(1+|g|) = 13.
#   GELU, b = 5:  inner = beta*fma(kappa, x^2*x, x): 5 relative.  t: b + 5*max|z|(1-tanh^2 z) = b + 2.25.
#     0.5*(1+t): (b+4.25)/2.  1-t*t: 2b+6.5.  beta*(1+3*kappa*x^2): 6 relative.  The product of the three factors and
#     the final add: (0.4*(2b+14.5) + 0.4)|x|(1+3 kappa x^2) + (b+4.25)/2 + 1  ->  at most 0.8b + 6.2 = 10.2.
#   dy*up and the product with act': 2 more.  max(13, 10.2) + 2 = 15, rounded up to a power of two.
D_GATE_C = 16


def d_gate_tol(gate, up, dy, act, ref, dt):
    """Largest |got - d_gate| a correct kernel leaves: one rounding to `dt`, D_GATE_C fp32 roundings of
    M = |dy*up|*(1 + |g|*(1 + 3*kappa*g^2 [GELU])), the size act' is assembled from, and the subnormal floor."""
    g, up, dy = f64(gate), f64(up), f64(dy)
    m = (dy * up).abs() * (1.0 + g.abs() * (1.0 + (3.0 * GELU_KAPPA * g * g if act == 1 else 0.0)))
    return unit_roundoff(dt) * ref.abs() + D_GATE_C * U32 * m + half_subnormal(dt)


def d_up_interval(gate, dy, act, a64, dt):
    """(lo, hi, ambiguous): d_up = dy * dt(act(gate)) with the activation rounded to `dt` first, as the forward kept
    it.  The kernel's fp32 activation is within e = 8*2^-24*(|act| + 0.5|g| [GELU]) of act64 -- GELU's 0.5*x*(1+t)
    loses 1+t to cancellation in the negative tail, where fp32 1+t is exactly 0 -- so its rounding is one of
    a_lo = dt(act64-e) .. a_hi = dt(act64+e); the result lies between dy*a_lo and dy*a_hi, each end widened by its own
    rounding to `dt` and the subnormal floor.  `ambiguous` marks the elements where a_lo != a_hi."""
    g, dy = f64(gate), f64(dy)
    u, fl = unit_roundoff(dt), half_subnormal(dt)
    e = 8.0 * U32 * (a64.abs() + (0.5 * g.abs() if act == 1 else 0.0))
    a_lo, a_hi = round_dt(a64 - e, dt), round_dt(a64 + e, dt)
    p, q = dy * a_lo, dy * a_hi
    lo, hi = torch.minimum(p, q), torch.maximum(p, q)
    return lo - (u * lo.abs() + fl), hi + (u * hi.abs() + fl), a_lo != a_hi


def rope_ref(q, cos, sin, sign, dt):
    """dt(dt(q*cos) + dt(rotate_half(q)*sign*sin)), rotate_half(q) = cat(-q2, q1); q (B,H,L,Dh), cos/sin (1|B,L,Dh), all
    values of `dt`; sign = -1 is the inverse rotation (the backward).  The kernel's rounding points: each product is
    exact in float64 and rounded once, the sum is an fp32 add rounded to `dt` -- so the comparison is bit for bit."""
    q, cos, sin = f64(q), f64(cos)[:, None], f64(sin)[:, None]
    h = q.shape[-1] // 2
    rot = torch.cat([-q[..., h:], q[..., :h]], -1)
    a = round_dt(q * cos, dt).to(torch.float32)
    b = round_dt(rot * float(sign) * sin, dt).to(torch.float32)
    return round_dt((a + b).double(), dt)


def _randn(shape, gen):
    return torch.randn(shape, generator=gen, dtype=torch.float32)


def norm_bwd_inputs(rows, D, dt, gemma, seed=0):
    """(x, w, dy, dsum) on the CPU in `dt`.  Row 0 is plain (x = 2*randn); of six rows the other five are: all zeros,
    x*1e-4 (eps dominates), x*100 (fp16 results near its subnormal range), one-hot (the two terms cancel to about
    D*eps/x0^2 of their size), and dy = 0.  w = 0.3*randn (+1 for Llama), so Gemma weights come near zero."""
    gen = torch.Generator().manual_seed(1000 * seed + D)
    x, dy, dsum = 2.0 * _randn((rows, D), gen), _randn((rows, D), gen), _randn((rows, D), gen)
    w = 0.3 * _randn((D,), gen) + (0.0 if gemma else 1.0)
    if rows >= 6:
        x[1] = 0.0
        x[2] *= 1e-4
        x[3] *= 100.0
        x[4, 1:] = 0.0
        x[4, 0] = 2.0
        dy[5] = 0.0
    return x.to(dt), w.to(dt), dy.to(dt), dsum.to(dt)


def gated_bwd_inputs(n, dt, seed=0):
    """(gate, up, dy) on the CPU in `dt`, n elements.  gate: an eighth on linspace(-30, 30), an eighth within 1e-2 of
    the zero of silu', an eighth within 1e-2 of the zero of gelu-tanh' (where the derivative's terms cancel), then
    0.0, -0.0, 88, -88 (saturated gates), the rest 4*randn; shuffled.  up = 2*randn, dy = randn."""
    gen = torch.Generator().manual_seed(2000 * seed + n % 9973)
    k = n // 8
    near = lambda z: z + 1e-2 * (2.0 * torch.rand(k, generator=gen, dtype=torch.float32) - 1.0)
    parts = [torch.linspace(-30.0, 30.0, k), near(SILU_DZERO), near(GELU_DZERO), torch.tensor([0.0, -0.0, 88.0, -88.0])]
    parts.append(4.0 * _randn((n - sum(p.numel() for p in parts),), gen))
    gate = torch.cat(parts)[torch.randperm(n, generator=gen)]
    return gate.to(dt), (2.0 * _randn((n,), gen)).to(dt), _randn((n,), gen).to(dt)


# the cases both test files run
NORM_BWD_D = {torch.bfloat16: [8, 256, 2048, 2056, 2560, 4096, 5120, 6152, 8192],     # 16-byte chunks per lane 1..4, full
              torch.float16: [8, 256, 2048, 2056, 2560, 4096, 5120, 6152, 8192],      # and partly filled last rounds
              torch.float32: [4, 128, 1024, 1028, 2560, 4096]}
NORM_BWD_EPS = {False: 1e-5, True: 1e-6}            # Llama's and Gemma's rms_norm_eps
GATED_BWD_N = [8, 24, 65536]                        # one chunk, three chunks, many workgroups
GATED_BWD_WRAP_N = (1048576 + 256 + 3) * 8          # bf16: past the 4096 x 256 chunks one pass of the backward's grid covers


def rope_inputs(B, H, L, Dh, cb, dt, seed=0):
    """(q, cos, sin, dq) on the CPU in `dt`: q and dq as strided (B,H,L,Dh) views of fused (B,L,3*H*Dh) projections,
    cos/sin (cb,L,Dh)."""
    gen = torch.Generator().manual_seed(seed + Dh + L)
    view = lambda t: t[..., H * Dh:2 * H * Dh].view(B, L, H, Dh).transpose(1, 2)
    q = view(_randn((B, L, 3 * H * Dh), gen).to(dt))
    dq = view(_randn((B, L, 3 * H * Dh), gen).to(dt))
    ang = torch.rand((cb, L, Dh // 2), generator=gen) * 6.28
    emb = torch.cat([ang, ang], -1)
    return q, emb.cos().to(dt), emb.sin().to(dt), dq


def rope_round_trip_tol(q, dt):
    """Largest |inverse(forward(x)) - x| per element, in roundings u of n = sqrt(x_i^2 + partner_i^2), the size of the
    pair the rotation mixes (it is orthogonal, so nothing grows): each pass rounds two products and their sum,
    u*(|x c| + |p s|) + u*|y| <= 2un; the forward's errors reach one output through c and s, (|c| + |s|)*2un <= 2*sqrt(2)*un;
    cos and sin are themselves rounded to the dtype, so c^2 + s^2 is 1 only to 2u.  2 + 2*sqrt(2) + 2 = 6.83, with the
    second-order terms 7.  (Two roundings are not enough: rope_ref itself reaches 3.97 on rope_inputs.)"""
    qd = f64(q)
    h = qd.shape[-1] // 2
    p = torch.cat([qd[..., h:], qd[..., :h]], -1)
    return 7.0 * unit_roundoff(dt) * torch.sqrt(qd * qd + p * p) + half_subnormal(dt)


def norm_bwd_ratio(got, x, w, dy, eps, gemma, dsum, dt) -> float:
    """Worst |got - ref| / bound over the elements: the check is `<= 1`."""
    ref = rmsnorm_bwd_ref(x, w, dy, eps, gemma, dsum)
    return ((f64(got) - ref.ref).abs() / norm_bwd_tol(ref, dt, dsum is not None)).max().item()


def gated_bwd_ratios(dg, du, gate, up, dy, act, dt):
    """(worst |d_gate error| / bound, worst distance of d_up from its interval's centre / half-width -- both checks are
    `<= 1` -- and the share of elements whose activation may round either way)."""
    a64, _, ref = gated_act_bwd_ref(gate, up, dy, act)
    rg = ((f64(dg) - ref).abs() / d_gate_tol(gate, up, dy, act, ref, dt)).max().item()
    lo, hi, amb = d_up_interval(gate, dy, act, a64, dt)
    ru = ((f64(du) - 0.5 * (lo + hi)).abs() / (0.5 * (hi - lo))).max().item()
    return rg, ru, amb.double().mean().item()


# --------------------------------------------------------------------------
# gradient-pass attention (csrc/causal_attention.hip: causal_fwd/dq/dkv_kernel; csrc/b1_attention.hip)
# --------------------------------------------------------------------------
# No reference program: attention and its backward in float64 on the 16-bit operands, and per ELEMENT the error a correct
# flash evaluation keeps.  The kernels round P and dS to the 16-bit type before their products and read delta from the
# rounded output; each of those roundings is relative to one term of a sum, so what one output element collects is
# u times the sum of the terms' sizes -- B below -- and, where a term falls into the type's subnormal range (fp16: P and
# dS of far keys), half a subnormal spacing per visible term -- Z.  A whole-tensor maximum would be set by the late
# queries and early keys, whose sums are long; these bounds shrink with the row.  Used by tests/test_attention_refs.py
# (CPU: against autograd, a restatement of the kernels, and mutants of it) and tests/test_attention_grad_gpu.py.
LOG2E = 1.4426950408889634
AttnRef = namedtuple("AttnRef", "o lse2 dq dk dv B Z")

# ATTN_C: the correct fp32 restatements of the kernels (tests/test_attention_refs.py: restate_causal, restate_b1) reach
# at most ATTN_WORST of the bound at C = 1 over every case of attention_cases(), ATTN_TWO_TILE_CASES and B1_S x B1_H, both
# dtypes, all input families; C is the smallest power of two >= 2 * that.  The factor of two is for what the restatements
# leave out: the order of the fp32 accumulation inside the matrix cores, v_exp_f32 / v_log_f32 being accurate to about
# an ulp.  Measured per output at C = 1 -- causal: o 0.83, dq 0.50, dk 0.94, dv 0.97; b1: o 0.94, dqkv 0.993 (a dv of the last key: one term, its P rounded, then the result).
# ATTN_C_LSE the same for the log-sum-exp against 2^-24 * max(1, |ref|), from ATTN_LSE_WORST (causal 26.3, b1 16.4: sharp
# fp16 rows of two or three keys whose lse2 is below one while sum |q_d k_d| scale log2(e) is about 40 -- the fp32 dot
# product's own error, relative to a result that cancelled).
ATTN_WORST = 0.993
ATTN_C = 2
ATTN_LSE_WORST = 26.3
ATTN_C_LSE = 64


def _visible(Lq, Lk, causal, device=None):
    """(Lq, Lk) bool: the queries are the LAST Lq positions, query i sees keys 0 .. Lk - Lq + i."""
    if not causal:
        return torch.ones((Lq, Lk), dtype=torch.bool, device=device)
    return torch.arange(Lk, device=device)[None, :] <= (Lk - Lq + torch.arange(Lq, device=device))[:, None]


def attention_ref(q, k, v, d_out, scale, causal, dt) -> AttnRef:
    """Attention of q (Lq,H,Dh) -- the last Lq positions -- over k / v (Lk,Hkv,Dh), query head h reading key/value head
    h // rep, and its backward for d_out (Lq,H,Dh), in float64 on operands already rounded to `dt`.  o, dq (Lq,H,Dh);
    dk, dv (Lk,Hkv,Dh) summed over the group; lse2 (H,Lq) = log2 of the denominator of the scaled scores.  B[name] and
    Z[name], shaped like the output: with p the probabilities, dP = dO.V^T and dabs_i = sum_d |dO_id||o_id| (what an
    error in the rounded o does to delta_i; |delta_i| itself would miss it, the sum over d cancels),
    A = p o (|dP| + dabs):   o: p.|v|   dv: p^T.|dO|   dq: scale A.|k|   dk: scale A^T.|q|;   Z the same with the 0/1
    visibility mask in place of p."""
    q, k, v, do = f64(q), f64(k), f64(v), f64(d_out)
    assert all(torch.equal(round_dt(t, dt), t) for t in (q, k, v, do)), "the operands must be values of dt"
    (Lq, H, Dh), (Lk, Hkv, _) = q.shape, k.shape
    rep = H // Hkv
    scale = float(np.float32(scale))                       # as the fp32 number the C entry point gets
    ke, ve = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
    vis = _visible(Lq, Lk, causal, q.device)
    s = (torch.einsum("qhd,khd->hqk", q, ke) * scale).masked_fill(~vis[None], float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = torch.einsum("hqk,khd->qhd", p, ve)
    dP = torch.einsum("qhd,khd->hqk", do, ve)
    delta = (do * o).sum(-1).t()[..., None]
    dS = p * (dP - delta) * scale
    group = lambda t: t.view(Lk, Hkv, rep, Dh).sum(2)      # noqa: E731
    dq = torch.einsum("hqk,khd->qhd", dS, ke)
    dk = group(torch.einsum("hqk,qhd->khd", dS, q))
    dv = group(torch.einsum("hqk,qhd->khd", p, do))
    mag = dP.abs() + (do.abs() * o.abs()).sum(-1).t()[..., None]
    B, Z = {}, {}
    for out, w in ((B, p), (Z, vis[None].to(torch.float64).expand_as(p))):
        a = w * mag * scale
        out["o"] = torch.einsum("hqk,khd->qhd", w, ve.abs())
        out["dv"] = group(torch.einsum("hqk,qhd->khd", w, do.abs()))
        out["dq"] = torch.einsum("hqk,khd->qhd", a, ke.abs())
        out["dk"] = group(torch.einsum("hqk,qhd->khd", a, q.abs()))
    return AttnRef(o, lse * LOG2E, dq, dk, dv, B, Z)


def attention_tol(ref: AttnRef, name, dt):
    """Largest |got - ref| a correct kernel leaves in output `name`, per element: ATTN_C roundings of the terms it sums
    (with their subnormal floors), and the one rounding of the result with its floor."""
    u, eta = unit_roundoff(dt), half_subnormal(dt)
    return ATTN_C * (u * ref.B[name] + eta * ref.Z[name]) + u * getattr(ref, name).abs() + eta


def lse_tol(ref_lse):
    return ATTN_C_LSE * U32 * ref_lse.abs().clamp_min(1.0)


def _worst(err, tol):
    r = err / tol
    i = int(r.argmax())
    return r.flatten()[i].item(), tuple(int(j) for j in np.unravel_index(i, tuple(r.shape)))


def attention_ratios(got, ref: AttnRef, dt):
    """{name: (worst |got - ref| / bound, the element where it occurs)} for the outputs given in the dict `got`
    (o, dq: (row, head, dim); dk, dv: (key, key/value head, dim); lse2: (head, row)): every check is `<= 1`.  A
    non-finite result counts as infinitely wrong."""
    out = {}
    for name, g in got.items():
        want = getattr(ref, name)
        err = torch.nan_to_num((f64(g).to(want.device) - want).abs(), nan=float("inf"))
        out[name] = _worst(err, lse_tol(want) if name == "lse2" else attention_tol(ref, name, dt))
    return out


B1Ref = namedtuple("B1Ref", "o lse dqkv tol_o tol_dqkv")


def _rot_partner(t):
    h = t.shape[-1] // 2
    return torch.cat([t[..., h:], t[..., :h]], -1)


def b1_attention_ref(qkv, cos, sin, H, scale, d_out, dt) -> B1Ref:
    """bma_b1_attention and its backward: qkv (S, 3*H*Dh) [q heads | k heads | v heads], cos / sin (S, Dh), d_out
    (S, H*Dh), all values of `dt`.  q and k are rotated with rope_ref (the kernel's rotation is bma_rope2's, bit for
    bit), attention_ref runs on the rotated operands, and dq' / dk' with their tolerances go back through the inverse
    rotation g_d = cos_d g'_d -+ sin_d g'_p (p the partner 64 away) exactly:
    tol_d = |cos_d| tol'_d + |sin_d| tol'_p + 3u (|cos_d g'_d| + |sin_d g'_p|) + 2 eta -- the kernel rounds dq' / dk' to
    `dt` first (that rounding is already in tol'), then the two products (relative u each, or half a subnormal spacing
    eta: without that floor a correct fp16 evaluation reaches 1.38 on a dk of order 1e-6, whatever C) and their sum.  o (S, H*Dh), lse (H, S) natural
    log, dqkv (S, 3*H*Dh) and the tolerances of o and dqkv, in the kernel's layouts."""
    S, Dh = qkv.shape[0], cos.shape[-1]
    q, k, v = (t.reshape(S, H, Dh) for t in f64(qkv).split(H * Dh, dim=-1))
    c, s = f64(cos).reshape(1, S, Dh), f64(sin).reshape(1, S, Dh)
    rot = lambda t, sign: rope_ref(t.transpose(0, 1)[None], c, s, sign, dt)[0].transpose(0, 1)      # noqa: E731
    ref = attention_ref(rot(q, 1.0), rot(k, 1.0), v, f64(d_out).reshape(S, H, Dh), scale, True, dt)
    u, eta = unit_roundoff(dt), half_subnormal(dt)
    cc, ss = c[0][:, None], s[0][:, None]                                   # (S, 1, Dh)
    sign = torch.cat([torch.ones(Dh // 2), -torch.ones(Dh // 2)]).to(cc)    # -(rotate_half's sign)
    grads, tols = [], []
    for name in ("dq", "dk"):
        g, t = getattr(ref, name), attention_tol(ref, name, dt)
        gp, tp = _rot_partner(g), _rot_partner(t)
        grads.append(cc * g + sign * ss * gp)
        tols.append(cc.abs() * t + ss.abs() * tp + 3.0 * u * ((cc * g).abs() + (ss * gp).abs()) + 2.0 * eta)
    grads.append(ref.dv)
    tols.append(attention_tol(ref, "dv", dt))
    flat = lambda ts: torch.cat([t.reshape(S, H * Dh) for t in ts], -1)      # noqa: E731
    return B1Ref(ref.o.reshape(S, H * Dh), ref.lse2 / LOG2E, flat(grads), attention_tol(ref, "o", dt).reshape(S, H * Dh), flat(tols))


def b1_attention_ratios(got, ref: B1Ref):
    """{name: (worst error / bound, element)} for `o` (row, column), `lse` (head, row) and `dqkv` (row, column: q heads |
    k heads | v heads) of the dict `got`."""
    tol = {"o": ref.tol_o, "dqkv": ref.tol_dqkv, "lse": lse_tol(ref.lse)}
    out = {}
    for name, g in got.items():
        want = getattr(ref, name)
        out[name] = _worst(torch.nan_to_num((f64(g).to(want.device) - want).abs(), nan=float("inf")), tol[name])
    return out


# ---- the cases both test files run ----
# (Lq, Lk) at 128-wide heads, H = Hkv = 2, causal: one key (dq and dk exactly zero, the odd-chunk half idle); one query
# behind a prefix; on and off the 16-row tile; around the 32-key chunk (33: a last chunk of one key, seen by one query);
# around the 64-row workgroup (65: a second workgroup of one row on both sides); even and odd chunk counts (the halves
# unequal); a prefix of exactly two chunks; diagonals that cross the chunks off their edges
ATTN_SHAPES = [(1, 1), (1, 33), (16, 16), (17, 17), (31, 31), (32, 32), (33, 33), (64, 64), (65, 65), (97, 97), (129, 129),
               (20, 84), (44, 107), (33, 98), (65, 200)]
ATTN_FAMILIES = ["randn", "sharp", "slow climb", "fast climb", "falling", "late outlier", "v ramp"]
AttnCase = namedtuple("AttnCase", "Lq Lk H Hkv Dh causal")
ATTN_TWO_TILE_CASES = [AttnCase(130, 130, 2, 2, 72, True), AttnCase(128, 128, 2, 2, 72, True), AttnCase(128, 128, 2, 2, 72, False)]


def attention_cases():
    """Every (Lq, Lk, H, Hkv, Dh, causal) of the per-element tests: ATTN_SHAPES, then four shapes each at the other head
    widths and for grouped heads, then every key visible."""
    cases = [AttnCase(Lq, Lk, 2, 2, 128, True) for Lq, Lk in ATTN_SHAPES]
    for Dh in (64, 72, 256):
        cases += [AttnCase(Lq, Lk, 2, 2, Dh, True) for Lq, Lk in ((33, 33), (65, 65), (44, 107), (65, 200))]
    for Hkv in (2, 1):
        cases += [AttnCase(Lq, Lk, 4, Hkv, 128, True) for Lq, Lk in ((17, 17), (129, 129), (33, 98), (65, 200))]
    cases += [AttnCase(Lq, Lk, 2, 2, 128, False) for Lq, Lk in ((33, 33), (65, 97), (100, 100))]
    return cases


B1_S = [1, 15, 16, 17, 31, 32, 33, 48, 65, 80]
B1_H = [1, 3]


def attention_inputs(case: AttnCase, dt, family, seed=0):
    """(q, k, v, d_out) on the CPU in `dt`.  randn: all four standard normal.  sharp: q times 4 -- the softmax is sharp,
    every row's output of order one, the dominant keys at random places in each row, so that a missing or leaked key
    moves some row grossly.  The four ramps add a score that depends on the key alone, through dim 0 of k (q[.., 0] = 1,
    0.25 on odd rows so that the lanes of one wave differ; the other dims small), in log2 units: +0.05 a key (the running
    maximum creeps up: alpha != 1 on every chunk), +0.4 a key (it jumps), -0.3 a key (it never moves after the first
    chunk: alpha == 1, and in fp16 far keys' P underflow), one key 40 above the rest near the end.  v ramp: randn with v
    scaled per key by linspace(0.5, 2), so that a permuted key order inside a k-step shows."""
    Lq, Lk, H, Hkv, Dh, _ = case
    gen = torch.Generator().manual_seed(100003 * seed + 1009 * Lq + 31 * Lk + 7 * Dh + H + 3 * Hkv + ATTN_FAMILIES.index(family))
    q, k, v, do = _randn((Lq, H, Dh), gen), _randn((Lk, Hkv, Dh), gen), _randn((Lk, Hkv, Dh), gen), _randn((Lq, H, Dh), gen)
    if family == "sharp":
        q = 4.0 * q
    elif family == "v ramp":
        v = v * torch.linspace(0.5, 2.0, Lk)[:, None, None]
    elif family != "randn":
        pos = torch.arange(Lk, dtype=torch.float32)
        ramp = {"slow climb": 0.05 * pos, "fast climb": 0.4 * pos, "falling": -0.3 * pos,
                "late outlier": 40.0 * (pos == (19 * Lk) // 20)}[family]
        k = 0.05 * k
        k[..., 0] = (ramp / (Dh ** -0.5 * LOG2E))[:, None]
        q = 0.5 * q
        q[..., 0] = 1.0
        q[(Lk - Lq + 1) % 2::2, :, 0] = 0.25          # odd POSITIONS
    return q.to(dt), k.to(dt), v.to(dt), do.to(dt)


def b1_inputs(S, H, dt, family, seed=0):
    """(qkv (S, 3*H*128) as a view of rows 64 elements wider, cos, sin (S, 128), d_out (S, H*128)) on the CPU in `dt`: the
    q, k, v of attention_inputs laid out as the fused projection's output, angles uniform in [0, 2 pi)."""
    q, k, v, do = attention_inputs(AttnCase(S, S, H, H, 128, True), dt, family, seed)
    gen = torch.Generator().manual_seed(977 * seed + S + 131 * H)
    ang = torch.rand((S, 64), generator=gen) * 6.28
    emb = torch.cat([ang, ang], -1)
    big = torch.zeros((S, 3 * H * 128 + 64), dtype=dt)
    big[:, :3 * H * 128] = torch.cat([t.reshape(S, H * 128) for t in (q, k, v)], -1)
    return big[:, :3 * H * 128], emb.cos().to(dt), emb.sin().to(dt), do.reshape(S, H * 128)
