"""The embedding-distance term of the token top-k on the MI355X: bma_token_dist_score against the float64 restatement of
the contract (token_dist_ref.py) through `ops` and once through the raw C ABI, its composition with bma_mask_topk, and whole
runs with ``token_dist_weight`` set on the tiny synthetic models.

What is compared how: every element of the kernel's output is held to its own bound 2^-24 * ((D/2 + 4) * w * d + 2 * |s|)
around the float64 value (token_dist_ref.bound: first-order rounding analysis for any summation order); NaN patterns and
infinities are compared exactly; the exact cases of the contract (the current token, duplicated table rows, the eighths
grid) bit for bit.  A top-k is compared with the float64 top-k wherever the float64 gaps exceed the two elements' bounds."""

import functools

import numpy as np
import pytest
import torch

import token_dist_ref as T
from mellowmax_ref import GOAL, MODES, TARGET, messages_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF, NAN = float("inf"), float("nan")
SENTINEL = 12345.0
WEIGHT = 0.3
RUN_CASES = T.RUN_CASES
COMBOS = [(e, g) for e in ("f32", "bf16", "f16") for g in ("f32", "bf16", "f16")]


def bits32(x) -> np.ndarray:
    return np.ascontiguousarray(x.detach().float().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float32)).view(np.int32)


def laid_out(grad, emb, rows, V, D):
    """The operands on the device in the awkward layouts: grad with ld_row = V + 3 starting one element off the 16-byte
    grid, the table with ld_emb = D + 8, out inside a larger sentinel-filled buffer with ld_out = V + 5."""
    gflat = torch.full((rows * (V + 3) + 16,), 7.0, dtype=grad.dtype, device=DEV)
    gview = gflat[1:1 + rows * (V + 3)].view(rows, V + 3)[:, :V]
    gview.copy_(grad)
    assert gview.data_ptr() % 16 == grad.element_size() and (rows == 1 or gview.stride(0) == V + 3)
    ebig = torch.full((V, D + 8), 9.0, dtype=emb.dtype, device=DEV)
    eview = ebig[:, :D]
    eview.copy_(emb)
    assert eview.data_ptr() % 16 == 0 and (V == 1 or eview.stride(0) == D + 8)
    obig = torch.full((rows + 2, V + 5), SENTINEL, dtype=torch.float32, device=DEV)
    return gview, eview, obig, obig[1:rows + 1, :V]


def sentinel_intact(obig, rows, V) -> bool:
    o = obig.cpu().numpy()
    return bool((o[0] == SENTINEL).all() and (o[rows + 1] == SENTINEL).all() and (o[1:rows + 1, V:] == SENTINEL).all())


def check_call(grad, emb, ids, weight, label=""):
    """One call through ops in the awkward layouts, every element against its bound; returns the output (numpy)."""
    from bimodalattack_amd import ops
    rows, V = grad.shape
    D = emb.shape[1]
    gview, eview, obig, oview = laid_out(grad, emb, rows, V, D)
    g0, e0 = gview.clone(), eview.clone()
    got = ops.token_dist_score(gview, eview, ids.to(DEV), weight, out=oview)
    assert got.data_ptr() == oview.data_ptr() and got.dtype == torch.float32
    torch.cuda.synchronize()
    assert sentinel_intact(obig, rows, V), "written outside out[0:rows, 0:V]"
    assert torch.equal(bits_of(gview), bits_of(g0)) and torch.equal(bits_of(eview), bits_of(e0)), "an input was modified"
    got = got.cpu().numpy()
    ref, bnd = T.restated64(grad, emb, ids, weight), T.bound(grad, emb, ids, weight)
    bad = T.outside(got, ref, bnd)
    fin = np.isfinite(ref)
    if fin.any():
        ratio = np.abs(got.astype(np.float64)[fin] - ref[fin]) / np.maximum(bnd[fin], 1e-300)
        print(f"{label} rows={rows} V={V} D={D} {emb.dtype}/{grad.dtype}: worst error / bound {ratio.max():.3f}")
    assert not bad.any(), (label, int(bad.sum()), np.argwhere(bad)[:5])
    return got


def bits_of(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ------------------------------------------------------------------ the kernel against the restatement
SHAPES = [(V, D) for V in (1, 63, 257, 4099) for D in (8, 72, 520)] + [(257, 4096)]


@pytest.mark.parametrize("V,D", SHAPES)
def test_kernel_equals_the_restatement(V, D):
    """rows in {1, 20, R, R + 1} (one group short, full, and a second group of one), every dtype pair over the cases
    (all nine at V = 63, D = 72), ids with 0, V - 1, a duplicate and one outside [0, V)."""
    case = SHAPES.index((V, D))
    for n, rows in enumerate((1, 20, T.R, T.R + 1)):
        combos = COMBOS if (V, D) == (63, 72) and rows == 20 else [COMBOS[(4 * case + n) % 9], COMBOS[(4 * case + n + 4) % 9]]
        if D >= 4096:
            combos = combos[:1]
        for ed, gd in combos:
            grad, emb, ids = T.generic_pool(rows, V, D, ed, gd, seed=n)
            if V > 8:
                emb, pairs = T.duplicate_rows(emb, ids)
            ids = ids.clone()
            if rows > 1:
                ids[1] = V if n % 2 else -1                                  # never read through: that row is NaN
            got = check_call(grad, emb, ids, WEIGHT, "generic")
            g32 = grad.float().numpy()
            for i, t in enumerate(ids.tolist()):
                if 0 <= t < V:
                    assert got[i, t].tobytes() == g32[i, t].tobytes(), "out[i, ids[i]] is the gradient, bit for bit"
                else:
                    assert np.isnan(got[i]).all()
            if V > 8:
                for i, v in pairs:
                    if 0 <= int(ids[i]) < V:
                        assert got[i, v].tobytes() == g32[i, v].tobytes(), "a duplicated row returns the gradient"


@pytest.mark.parametrize("dt", sorted(T.DTYPES))
@pytest.mark.parametrize("rows,V,D", [(1, 1, 8), (20, 257, 72), (33, 63, 520), (5, 4099, 264)])
def test_exact_grid_bit_for_bit(rows, V, D, dt):
    grad, emb, ids, w = T.grid_pool(rows, V, D)
    want = T.restated64(grad, emb, ids, w).astype(np.float32)
    got = check_call(grad.to(T.DTYPES[dt]), emb.to(T.DTYPES[dt]), ids, w, "grid")
    assert np.array_equal(bits32(got), bits32(want))


@pytest.mark.parametrize("ed,gd", [("f32", "bf16"), ("bf16", "f32"), ("f16", "f16")])
def test_weight_zero_returns_the_gradient(ed, gd):
    from bimodalattack_amd import ops
    grad, emb, ids = T.generic_pool(20, 257, 72, ed, gd)
    out = ops.token_dist_score(grad.to(DEV), emb.to(DEV), ids.to(DEV), 0.0)
    assert np.array_equal(bits32(out), bits32(grad.float()))
    two = ops.token_dist_score(grad.to(DEV), emb.to(DEV), ids.to(DEV), 0.0)
    assert np.array_equal(bits32(out), bits32(two))


@pytest.mark.parametrize("dt", sorted(T.DTYPES))
def test_special_values(dt):
    """NaN and inf in the table and in the gradient propagate as IEEE arithmetic gives them -- inf - inf in a difference,
    0 * inf with weight 0 -- and a negative-zero gradient at the current token comes out as g + 0.0."""
    from bimodalattack_amd import ops
    dtype = T.DTYPES[dt]
    grad, emb, ids = T.generic_pool(6, 130, 264, dt, dt)
    emb, grad, ids = emb.clone(), grad.clone(), ids.clone()
    emb[3, 2] = INF
    emb[4, 200] = -INF
    emb[5, 1] = NAN
    emb[6, 263] = INF
    emb[7, 263] = INF                       # row 7 - row 6: inf - inf
    ids[3] = 6
    grad[0, 9] = INF
    grad[1, 10] = NAN
    grad[2, 11] = -INF
    grad[0, 0] = -0.0                       # ids[0] == 0
    for w in (WEIGHT, 0.0):
        ref = T.restated64(grad, emb, ids, w)
        got = check_call(grad, emb, ids, w, f"special w={w}")
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.isnan(ref[3, 7]) and np.isnan(ref[0, 5]) and np.isnan(ref[2, 5]) and ref[2, 11] == -INF
        assert (ref[0, 3] == INF) == (w > 0) and np.isnan(ref[0, 3]) == (w == 0)
        assert got[0, 0] == 0.0
    assert dtype in (torch.float32, torch.bfloat16, torch.float16)


def test_raw_c_abi():
    """bma_token_dist_score itself, with the awkward leading dimensions, a gradient off the 16-byte grid, two groups of
    rows, and an id outside the table."""
    from bimodalattack_amd import native, ops
    rows, V, D = T.R + 3, 257, 72
    grad, emb, ids = T.generic_pool(rows, V, D, "bf16", "f16")
    ids = ids.clone()
    ids[T.R + 1] = V + 7
    gview, eview, obig, oview = laid_out(grad, emb, rows, V, D)
    idd = ids.to(DEV)
    rc = native.lib.bma_token_dist_score(gview.data_ptr(), V + 3, rows, V, 2, eview.data_ptr(), D + 8, D, 1, idd.data_ptr(),
                                         WEIGHT, oview.data_ptr(), V + 5, ops._stream(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    assert sentinel_intact(obig, rows, V)
    got = oview.cpu().numpy()
    ref, bnd = T.restated64(grad, emb, ids, WEIGHT), T.bound(grad, emb, ids, WEIGHT)
    assert not T.outside(got, ref, bnd).any() and np.isnan(got[T.R + 1]).all() and np.isfinite(got[T.R + 2]).all()
    # the misaligned table is refused by the library itself, and nothing is written
    assert native.lib.bma_token_dist_score(gview.data_ptr(), V + 3, rows, V, 2, eview.data_ptr() + 2, D + 8, D, 1, idd.data_ptr(),
                                           WEIGHT, oview.data_ptr(), V + 5, ops._stream(torch.device(DEV))) == -3


def test_wrapper_checks_and_fallbacks():
    from bimodalattack_amd import ops
    grad, emb, ids = T.generic_pool(4, 40, 24, "bf16", "f32")
    g, e, i = grad.to(DEV), emb.to(DEV), ids.to(DEV)
    ref, bnd = T.restated64(grad, emb, ids, WEIGHT), T.bound(grad, emb, ids, WEIGHT)
    for bad in (-1.0, -INF, INF, NAN, True, "1"):
        with pytest.raises(ValueError, match="weight"):
            ops.token_dist_score(g, e, i, bad)
    with pytest.raises(ValueError):
        ops.token_dist_score(g[0], e, i, WEIGHT)
    with pytest.raises(ValueError):
        ops.token_dist_score(g, e[:39], i, WEIGHT)
    with pytest.raises(ValueError):
        ops.token_dist_score(g, e, i[:3], WEIGHT)
    with pytest.raises(ValueError):
        ops.token_dist_score(g, e, i.int(), WEIGHT)
    with pytest.raises(ValueError):
        ops.token_dist_score(g, e[:, :20], i, WEIGHT)                    # 40-byte rows: not a multiple of 16
    with pytest.raises(TypeError):
        ops.token_dist_score(g.double(), e, i, WEIGHT)
    with pytest.raises(ValueError, match="out"):
        ops.token_dist_score(g, e, i, WEIGHT, out=torch.empty(4, 40, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(ValueError, match="out"):
        ops.token_dist_score(g, e, i, WEIGHT, out=torch.empty(40, 4, dtype=torch.float32, device=DEV).t())
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        ops.token_dist_score(g.cpu(), e.cpu(), i.cpu(), WEIGHT)
    # a last stride that is not 1, a table off the 16-byte grid: the wrapper makes contiguous copies
    turned = g.t().contiguous().t()
    shifted = torch.empty(40 * 24 + 8, dtype=e.dtype, device=DEV)[4:4 + 40 * 24].view(40, 24)
    shifted.copy_(e)
    assert turned.stride(1) != 1 and shifted.data_ptr() % 16 == 8
    for gg, ee in ((turned, e), (g, shifted), (g, e.t().contiguous().t())):
        assert not T.outside(ops.token_dist_score(gg, ee, i, WEIGHT).cpu().numpy(), ref, bnd).any()


# ------------------------------------------------------------------ composition with the top-k
@pytest.mark.parametrize("V,D,k,dt", [(257, 72, 16, "f32"), (5000, 40, 32, "bf16")])
def test_composition_with_mask_topk(V, D, k, dt):
    """mask_topk(token_dist_score(...)) is the top-k of the float64 score ordered by (score, id), on a pool whose float64
    gaps -- at the k boundary and between neighbours inside the top-k -- exceed the two elements' bounds at every row
    (checked here, on the CPU: the pool needs no exclusion).  V = 5000 takes the two-stage select."""
    from bimodalattack_amd import ops
    rows = 20
    grad, emb, ids = T.generic_pool(rows, V, D, dt, dt, seed=3)
    banned = np.arange(0, V, 7)
    ref, bnd = T.restated64(grad, emb, ids, WEIGHT), T.bound(grad, emb, ids, WEIGHT)
    assert not T.fragile_rows(ref, bnd, k, banned, ordered=True).any()
    want = T.topk64(ref, k, banned)[0]
    bits = ops.build_mask_bits(torch.from_numpy(banned), V, DEV)
    score = ops.token_dist_score(grad.to(DEV), emb.to(DEV), ids.to(DEV), WEIGHT)
    got = ops.mask_topk(score, bits, k).cpu().numpy()
    assert np.array_equal(got, want)
    assert not np.array_equal(want, T.topk64(grad.double().numpy(), k, banned)[0])          # the term is not idle


# ------------------------------------------------------------------ whole runs
K_RUN = 16


def run_config(mode, steps=4):
    import tempfile
    from bimodalattack_amd import GCGConfig, synthetic as S
    return GCGConfig(seed=1, verbosity="ERROR", optim_str_init=S.TINY_OPTIM_INIT, images_folder=tempfile.mkdtemp(prefix="bma_td_"),
                     **{**MODES[mode], "num_steps": steps, "topk": K_RUN})


def run_td(kind, mode, steps=4, trace=True, **engine):
    from bimodalattack_amd import run, synthetic as S
    model, tok, proc, image = S.tiny_case(kind, device=DEV)
    cfg = run_config(mode, steps)
    tr = [] if trace else None
    res = run(model, tok, proc, messages_for(kind, mode), GOAL, TARGET, image if cfg.pgd_attack else None, cfg,
              normalize=S.Normalize(S.CLIP_MEAN, S.CLIP_STD), rng_device="cpu", trace=tr, strict=True, save_images=False, **engine)
    return res, tr


@functools.lru_cache(maxsize=None)
def _table(kind):
    from bimodalattack_amd import synthetic as S
    from bimodalattack_amd.utils import get_nonascii_toks
    model, tok, _, _ = S.tiny_case(kind)
    emb = model.get_input_embeddings()
    scale = getattr(emb, "embed_scale", None)
    scale = 1.0 if scale is None else float(torch.as_tensor(scale).to(emb.weight.dtype).float())
    return emb.weight.detach(), scale, get_nonascii_toks(tok).numpy()


@functools.lru_cache(maxsize=None)
def _plain_run(kind, mode):
    return run_td(kind, mode)


@functools.lru_cache(maxsize=None)
def _nearest(kind, mode):
    """(a): one traced run at weight 1e6; returns (pairs left out, pairs)."""
    E, scale, banned = _table(kind)
    res, trace = run_td(kind, mode, token_dist_weight=1e6)
    assert len(trace) == 4
    left, pairs = 0, 0
    for n, st in enumerate(trace):
        assert st["token_dist_weight"] == T.w32(1e6 * scale)
        g, ids = st["grad_tok"][-1], st["optim_ids_in"][0]
        ref, bnd = T.restated64(g, E, ids, st["token_dist_weight"]), T.bound(g, E, ids, st["token_dist_weight"])
        frag = T.fragile_rows(ref, bnd, K_RUN, banned, ordered=False)
        near = T.topk64(T.distance64(E, ids), K_RUN, banned)[0]
        assert st["topk_idx"].shape == near.shape
        for i in np.nonzero(~frag)[0]:
            assert set(st["topk_idx"][i]) == set(near[i]), (kind, mode, n, i)
        left += int(frag.sum())
        pairs += frag.size
    return left, pairs


@pytest.mark.parametrize("kind,mode", RUN_CASES)
def test_run_with_a_huge_weight_draws_from_the_nearest_tokens(kind, mode):
    _nearest(kind, mode)


def test_nearest_runs_leave_out_few_pairs():
    tot = np.sum([_nearest(kind, mode) for kind, mode in RUN_CASES], axis=0)
    print(f"(a) pairs left out: {tot[0]} of {tot[1]}")
    assert tot[0] <= 0.05 * tot[1]


@functools.lru_cache(maxsize=None)
def _moderate(kind, mode):
    """(b): the weight derived from the weight-0 run's trace; one traced run with it.  Returns (pairs left out, pairs, steps
    whose top-k sets differ from the weight-0 run's, pairs at which the score WITHOUT emb_scale has another top-k)."""
    E, scale, banned = _table(kind)
    _, plain = _plain_run(kind, mode)
    assert all("token_dist_weight" not in st for st in plain)
    w = T.moderate_weight(plain, E, scale)
    res, trace = run_td(kind, mode, token_dist_weight=w)
    left, pairs, changed, unscaled = 0, 0, 0, 0
    for n, st in enumerate(trace):
        w_eff = st["token_dist_weight"]
        assert w_eff == T.w32(w * scale)
        g, ids = st["grad_tok"][-1], st["optim_ids_in"][0]
        ref, bnd = T.restated64(g, E, ids, w_eff), T.bound(g, E, ids, w_eff)
        frag = T.fragile_rows(ref, bnd, K_RUN, banned, ordered=True)
        want = T.topk64(ref, K_RUN, banned)[0]
        mutant = T.topk64(T.restated64(g, E, ids, w), K_RUN, banned)[0]
        for i in np.nonzero(~frag)[0]:
            assert np.array_equal(st["topk_idx"][i], want[i]), (kind, mode, n, i)
            unscaled += not np.array_equal(st["topk_idx"][i], mutant[i])
        changed += any(set(a) != set(b) for a, b in zip(st["topk_idx"], plain[n]["topk_idx"]))
        left += int(frag.sum())
        pairs += frag.size
    print(f"(b) {kind}/{mode}: weight {w:.4g}, left out {left} of {pairs}, steps with another top-k than weight 0: {changed}")
    return left, pairs, changed, unscaled


@pytest.mark.parametrize("kind,mode", RUN_CASES)
def test_run_with_a_moderate_weight_ranks_the_restated_score(kind, mode):
    left, pairs, changed, unscaled = _moderate(kind, mode)
    assert changed >= 1, "the weight changes no top-k: the test shows nothing"
    if kind == "gemma3":
        assert unscaled >= 1, "(d) the score without emb_scale has the same top-k everywhere"
    else:
        assert unscaled == 0                                              # emb_scale == 1: the same score


def test_moderate_runs_leave_out_few_pairs():
    tot = np.sum([_moderate(kind, mode)[:2] for kind, mode in RUN_CASES], axis=0)
    print(f"(b) pairs left out: {tot[0]} of {tot[1]}")
    assert tot[0] <= 0.05 * tot[1]


@pytest.mark.parametrize("kind,mode", [("llava", "gcg"), ("gemma3", "joint")])
def test_weight_zero_is_the_default_path(kind, mode):
    """(c) token_dist_weight = 0.0 and the option absent: identical losses and strings, and by the profile counters the
    kernel is never launched (with a weight it is, once per step)."""
    from bimodalattack_amd import native
    base, _ = _plain_run(kind, mode)
    native.profile_enable(True)
    try:
        zero, _ = run_td(kind, mode, trace=False, token_dist_weight=0.0)
        assert native.profile_read()["token_dist"]["launches"] == 0
        native.profile_enable(True)
        run_td(kind, mode, trace=False, token_dist_weight=0.5)
        prof = native.profile_read()
        assert prof["token_dist"]["launches"] == 4 and prof["token_dist"]["symbol"] == "token_dist_kernel"
    finally:
        native.profile_enable(False)
    assert zero.losses == base.losses and zero.strings == base.strings


@pytest.mark.parametrize("mode", ["gcg", "joint"])
def test_no_host_reads_added(mode):
    """(e) the option adds no host synchronisation per step."""
    from test_apgd_gpu import _HostReads
    counts = {}
    for w in (0.0, 0.5):
        run_td("llava", mode, steps=2, trace=False, token_dist_weight=w, filter_first=False)       # warm
        with _HostReads() as h:
            run_td("llava", mode, steps=6, trace=False, token_dist_weight=w, filter_first=False)
        counts[w] = h.n
    assert counts[0.5] == counts[0.0], counts
