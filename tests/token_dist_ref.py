"""References of the embedding-distance term of the token top-k (EngineOptions.token_dist_weight; contract in
include/bma.h, a3b) for test_token_dist.py and test_token_dist_gpu.py: the float64 restatement of the contract, its
per-element rounding bound, float32 restatements of the kernel's arithmetic in two summation orders, the mutants the
tests tell apart from the rule, seeded input pools, and the top-k of a score matrix with its tie-exclusion rule.  No
kernel is touched here.

Conventions: `grad` (rows, V) and `emb` (V, D) are numpy arrays or torch tensors holding values that are ALREADY rounded to
their dtype (float32 / bfloat16 / float16); everything is widened exactly.  `weight` is rounded to float32 first, as the
launch argument is.  An id outside [0, V) gives a row of NaN."""

import numpy as np
import torch

R = 32                                  # BMA_TOKEN_DIST_ROWS: suffix positions per pass over the table
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
EPS = 2.0 ** -24
# the whole runs of both test files: tiny_case kinds x modes (the OPT model has no vision tower, so no joint mode)
RUN_CASES = [("opt", "gcg"), ("llava", "gcg"), ("llava", "joint"), ("gemma3", "gcg"), ("gemma3", "joint")]


def _np64(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().double().numpy()
    return np.asarray(x, np.float64)


def _np32(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().float().numpy()
    return np.asarray(x, np.float32)


def _ids(ids) -> np.ndarray:
    return ids.detach().cpu().numpy().astype(np.int64) if isinstance(ids, torch.Tensor) else np.asarray(ids, np.int64)


def w32(weight: float) -> float:
    return float(np.float32(weight))


# ------------------------------------------------------------------------------------------------- the rule, restated
def distance64(emb, ids) -> np.ndarray:
    """(rows, V) float64 distances ||E[v] - E[ids[i]]||_2 in the difference form; NaN rows for ids outside [0, V)."""
    E, ids = _np64(emb), _ids(ids)
    V = E.shape[0]
    ok = (ids >= 0) & (ids < V)
    d = np.full((ids.size, V), np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in np.nonzero(ok)[0]:
            diff = E - E[ids[i]][None, :]
            d[i] = np.sqrt((diff * diff).sum(-1))
    return d


def restated64(grad, emb, ids, weight) -> np.ndarray:
    """The contract in float64: grad[i, v] + float32(weight) * ||E[v] - E[ids[i]]||_2."""
    with np.errstate(invalid="ignore", over="ignore"):
        return _np64(grad) + w32(weight) * distance64(emb, ids)


def bound(grad, emb, ids, weight) -> np.ndarray:
    """The per-element bound 2^-24 * ((D/2 + 4) * weight * d64 + 2 * |s64|): first-order rounding analysis of the contract's
    arithmetic for ANY summation order -- per term one rounding of the difference (it enters squared: two) and one of the
    square, at most D - 1 of the additions: <= D + 2 relative roundings on the sum of squares, halved by the square root;
    then one rounding each for the square root, the product and the add (the last relative to |s|).  The slack is the + 1
    and the factor 2.  NaN where the restatement is not finite."""
    D = _np64(emb).shape[1]
    d = distance64(emb, ids)
    with np.errstate(invalid="ignore", over="ignore"):
        s = _np64(grad) + w32(weight) * d
        b = EPS * ((D / 2 + 4) * w32(weight) * d + 2 * np.abs(s))
    return np.where(np.isfinite(s), b, np.nan)


def restated32(grad, emb, ids, weight, order="sequential", fma=False) -> np.ndarray:
    """The kernel's arithmetic in float32 (numpy rounds every operation): differences, squares, the sum over c in column
    order ("sequential") or as a balanced tree over the zero-padded columns ("pairwise"), sqrt, weight * d, + g."""
    f32 = np.float32
    g, E, ids = _np32(grad), _np32(emb), _ids(ids)
    V, D = E.shape
    w = f32(weight)
    out = np.full(g.shape, np.nan, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(ids.size):
            if not 0 <= ids[i] < V:
                continue
            diff = (E - E[ids[i]][None, :]).astype(f32)
            sq = (diff * diff).astype(f32)
            if order == "sequential":
                acc = np.zeros(V, f32)
                for c in range(D):
                    acc = (acc + sq[:, c]).astype(f32)
            else:
                n = 1
                while n < D:
                    n *= 2
                t = np.zeros((V, n), f32)
                t[:, :D] = sq
                while n > 1:
                    n //= 2
                    t = (t[:, :n] + t[:, n:2 * n]).astype(f32)
                acc = t[:, 0]
            d = np.sqrt(acc).astype(f32)
            out[i] = (g[i] + (w * d).astype(f32)).astype(f32)
    return out


# ------------------------------------------------------------------------------------------------------- the mutants
def mutant_squared(grad, emb, ids, weight):
    """The squared distance in place of the distance."""
    d = distance64(emb, ids)
    return _np64(grad) + w32(weight) * d * d


def mutant_next_id(grad, emb, ids, weight):
    """The distance to the NEXT position's token (ids[i + 1], cyclically)."""
    return restated64(grad, emb, np.roll(_ids(ids), -1), weight)


def mutant_weight_on_grad(grad, emb, ids, weight):
    """The weight applied to the gradient instead of to the distance."""
    return w32(weight) * _np64(grad) + distance64(emb, ids)


def mutant_norm_expansion(grad, emb, ids, weight):
    """||a||^2 + ||b||^2 - 2 a.b in float32 (clamped at 0 before the root), the form the contract rules out.  As in a kernel
    that takes the norms from one pass and the products from another, the two are summed in different orders (the norms
    column by column, the products as numpy's pairwise sum): the three terms then do not cancel where the distance is 0 --
    at v = ids[i] and at duplicated table rows the result is the gradient plus rounding residue of the norms' size."""
    f32 = np.float32
    g, E, ids = _np32(grad), _np32(emb), _ids(ids)
    n2 = np.cumsum((E * E).astype(f32), axis=-1, dtype=f32)[:, -1]
    out = np.empty(g.shape, f32)
    for i in range(ids.size):
        dot = (E * E[ids[i]][None, :]).astype(f32).sum(-1, dtype=f32)
        sq = np.maximum((n2 + n2[ids[i]]).astype(f32) - (f32(2) * dot).astype(f32), f32(0))
        out[i] = g[i] + f32(weight) * np.sqrt(sq).astype(f32)
    return out


def outside(got, ref, bnd) -> np.ndarray:
    """Boolean mask of the elements of `got` that leave the bound around `ref` (NaN patterns must agree exactly)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    bad = np.zeros(ref.shape, bool)
    with np.errstate(invalid="ignore"):
        bad[fin] = ~(np.abs(got[fin] - ref[fin]) <= bnd[fin])
    bad[~fin] = ~((np.isnan(got[~fin]) & np.isnan(ref[~fin])) | (got[~fin] == ref[~fin]))
    return bad


# ------------------------------------------------------------------------------------------------------------- inputs
def ids_for(rows: int, V: int, seed: int = 0) -> np.ndarray:
    """Seeded current tokens with the placements that matter: 0, V - 1 and a duplicate."""
    ids = np.random.RandomState(50 + seed + 7 * rows + V).randint(0, V, size=rows).astype(np.int64)
    ids[0] = 0
    if rows > 1:
        ids[-1] = V - 1
    if rows > 3:
        ids[2] = ids[1]
    return ids


def generic_pool(rows: int, V: int, D: int, edtype="f32", gdtype="f32", seed: int = 0, offset: float = 0.0):
    """(grad, emb, ids) as torch CPU tensors of the two dtypes: a table like an embedding (normal, sigma 0.05, plus
    `offset` in every element), a gradient like a token gradient (normal, sigma 0.02), values that round everywhere."""
    rs = np.random.RandomState(4000 + seed + 31 * rows + 7 * V + D)
    emb = torch.from_numpy((offset + 0.05 * rs.standard_normal((V, D))).astype(np.float32)).to(DTYPES[edtype])
    grad = torch.from_numpy((0.02 * rs.standard_normal((rows, V))).astype(np.float32)).to(DTYPES[gdtype])
    return grad, emb, torch.from_numpy(ids_for(rows, V, seed))


def duplicate_rows(emb: torch.Tensor, ids: torch.Tensor, seed: int = 0):
    """A copy of the table in which, for every position whose vocabulary allows it, one more row equals row ids[i] bit for
    bit; returns (table, list of (i, v) pairs with v != ids[i] and row v == row ids[i])."""
    emb = emb.clone()
    V = emb.shape[0]
    used = set(int(t) for t in ids)
    pairs = []
    rs = np.random.RandomState(77 + seed)
    for i, t in enumerate(ids.tolist()):
        free = [v for v in rs.permutation(V)[:8].tolist() if v not in used]
        if free:
            emb[free[0]] = emb[t]
            used.add(free[0])
            pairs.append((i, free[0]))
    return emb, pairs


def grid_pool(rows: int, V: int, D: int, seed: int = 0):
    """(grad, emb, ids, weight) on which every intermediate of the contract is representable in float32 (and the inputs in
    bfloat16 and float16): table rows c_v * u with u a 0/1 vector of four ones and c_v on eighths in [-8, 8), so the
    distance is 2 * |c_v - c_x|, a multiple of 1/4 below 32; the gradient on eighths in [-4, 4); weight 0.375.  Any
    summation order gives the same bits, and restated32 == restated64 bit for bit."""
    assert D >= 4
    rs = np.random.RandomState(6000 + seed + 31 * rows + 7 * V + D)
    u = np.zeros(D, np.float32)
    u[rs.permutation(D)[:4]] = 1.0
    c = (rs.randint(-64, 64, size=V) / 8.0).astype(np.float32)
    emb = torch.from_numpy(c[:, None] * u[None, :])
    grad = torch.from_numpy((rs.randint(-32, 32, size=(rows, V)) / 8.0).astype(np.float32))
    return grad, emb, torch.from_numpy(ids_for(rows, V, seed)), 0.375


# ------------------------------------------------------------------------------------------------------------- top-k
def topk64(score64: np.ndarray, k: int, not_allowed=None):
    """Per row the k allowed tokens with the smallest score, ordered by (score, id) -- bma_mask_topk's order, NaN first --
    and, per row, the float64 gaps between neighbours of that order at positions 0..k (gap[j] = s[j + 1] - s[j]; the last
    one is the gap at the k boundary).  Rows need V - masked > k."""
    s = np.array(score64, np.float64)
    if not_allowed is not None and len(not_allowed):
        s[:, np.asarray(not_allowed)] = np.inf
    order = np.lexsort((np.broadcast_to(np.arange(s.shape[1]), s.shape), np.where(np.isnan(s), -np.inf, s)), axis=-1)
    top = order[:, :k + 1]
    vals = np.take_along_axis(s, top, -1)
    with np.errstate(invalid="ignore"):
        return order[:, :k], vals[:, 1:] - vals[:, :-1], top


def fragile_rows(score64: np.ndarray, bnd: np.ndarray, k: int, not_allowed=None, ordered=True) -> np.ndarray:
    """Rows whose top-k a float32 evaluation inside `bnd` may legitimately change: the float64 gap at the k boundary -- with
    `ordered`, also a gap between neighbours inside the top-k -- does not exceed the sum of the two elements' bounds."""
    idx, gaps, top = topk64(score64, k, not_allowed)
    b = np.take_along_axis(bnd, top, -1)
    with np.errstate(invalid="ignore"):
        close = ~(gaps > b[:, 1:] + b[:, :-1])
    return close.any(-1) if ordered else close[:, -1]


def moderate_weight(trace, emb, emb_scale: float) -> float:
    """The weight of the whole-run tests' moderate case, derived from the trace of a weight-0 run and the table: the one at
    which the distance term is of the order of the recorded gradients' spread,
        weight * emb_scale * median_{i, v} ||E[v] - E[x_i]||  =  std over (step, i, v) of grad_tok,
    with x the first step's tokens.  (The engine multiplies by emb_scale itself.)"""
    g = np.concatenate([np.asarray(st["grad_tok"][-1], np.float64).ravel() for st in trace])
    d = distance64(emb, np.asarray(trace[0]["optim_ids_in"]).reshape(-1))
    return float(g.std() / (float(emb_scale) * np.median(d[d > 0])))
