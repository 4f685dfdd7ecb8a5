"""The embedding-distance term of the token top-k (EngineOptions.token_dist_weight; include/bma.h, a3b), everything that
needs no GPU: the float64 restatement against torch, the rounding bound against float32 restatements in two summation
orders, the mutants the bound tells apart, the exact grid, the option, the C entry point's argument checks, and the
conditions the GPU whole-run tests rely on, established here on the CPU reference alone."""

import copy
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch

import token_dist_ref as T
from mellowmax_ref import GOAL, MODES, TARGET, messages_for

INF, NAN = float("inf"), float("nan")

# (rows, V, D, edtype, gdtype, table offset): the pools of the bound test and of the mutants
POOLS = [(5, 63, 8, "f32", "f32", 0.0), (20, 257, 72, "bf16", "bf16", 0.0), (3, 130, 520, "f16", "f32", 0.0),
         (7, 96, 72, "f32", "bf16", 4.0), (33, 40, 24, "bf16", "f16", 1.0)]
WEIGHT = 0.3


@functools.lru_cache(maxsize=None)
def _pool(spec):
    rows, V, D, ed, gd, off = spec
    grad, emb, ids = T.generic_pool(rows, V, D, ed, gd, offset=off)
    emb, pairs = T.duplicate_rows(emb, ids)
    return grad, emb, ids, pairs, T.restated64(grad, emb, ids, WEIGHT), T.bound(grad, emb, ids, WEIGHT)


# ------------------------------------------------------------------------------------------------ restatement, bound
def test_restatement_equals_torch_in_float64():
    """restated64 against torch.cdist in float64 (the difference form, no matrix product), and against the objective it
    linearises: with L(p) = sum_i <g_i, p_i> + w * sum_i ||p_i E - E[x_i]||_2 on one-hot rows p_i, moving position i from
    its current token to v changes L by exactly score[i, v] - score[i, x_i]."""
    for spec in POOLS[:3]:
        grad, emb, ids, _, ref, _ = _pool(spec)
        E = emb.double()
        d = torch.cdist(E[ids], E, compute_mode="donot_use_mm_for_euclid_dist").numpy()
        want = grad.double().numpy() + T.w32(WEIGHT) * d
        np.testing.assert_allclose(ref, want, rtol=1e-13, atol=1e-300)
    grad, emb, ids, _, ref, _ = _pool(POOLS[0])
    g, E, w = grad.double(), emb.double(), T.w32(WEIGHT)
    V = E.shape[0]

    def L(tokens):
        p = torch.nn.functional.one_hot(tokens, V).double()
        return float((g * p).sum() + w * ((p @ E) - E[ids]).norm(dim=-1).sum())
    base = L(ids)
    for i, v in ((0, 5), (2, V - 1), (4, 0), (1, int(ids[1]))):
        moved = ids.clone()
        moved[i] = v
        assert abs((L(moved) - base) - (ref[i, v] - ref[i, int(ids[i])])) <= 1e-13


@pytest.mark.parametrize("order", ["sequential", "pairwise"])
@pytest.mark.parametrize("spec", POOLS)
def test_float32_restatements_stay_inside_the_bound(spec, order):
    grad, emb, ids, pairs, ref, bnd = _pool(spec)
    got = T.restated32(grad, emb, ids, WEIGHT, order)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{spec} {order}: worst error / bound {np.max(err / bnd):.3f}")
    assert not T.outside(got, ref, bnd).any()
    # the exact cases of the contract: the current token and duplicated rows return the gradient, bit for bit
    g32 = grad.float().numpy()
    for i, t in enumerate(ids.tolist()):
        assert got[i, t].tobytes() == g32[i, t].tobytes() and bnd[i, t] == 2 * T.EPS * abs(float(g32[i, t]))
    assert pairs
    for i, v in pairs:
        assert got[i, v].tobytes() == g32[i, v].tobytes()


def test_out_of_range_ids_and_special_values_in_the_restatements():
    grad, emb, ids = T.generic_pool(4, 20, 8)
    ids = ids.clone()
    ids[1] = 20
    ids[2] = -1
    emb = emb.clone()
    emb[3, 2] = INF
    emb[4, 1] = NAN
    grad = grad.clone()
    grad[0, 7] = -INF
    ref, r32 = T.restated64(grad, emb, ids, WEIGHT), T.restated32(grad, emb, ids, WEIGHT)
    assert np.isnan(ref[1]).all() and np.isnan(ref[2]).all() and np.isnan(r32[1]).all() and np.isnan(r32[2]).all()
    assert ref[0, 3] == INF and np.isnan(ref[0, 4]) and ref[0, 7] == -INF and np.isfinite(ref[3, [0, 1, 2, 5]]).all()
    assert not T.outside(r32, ref, T.bound(grad, emb, ids, WEIGHT)).any()
    zero = T.restated64(grad, emb, ids, 0.0)                      # weight 0 follows IEEE: 0 * inf = NaN
    assert np.isnan(zero[0, 3]) and np.isnan(zero[0, 4]) and zero[0, 5] == float(grad[0, 5])


# ------------------------------------------------------------------------------------------------------- mutants
@pytest.mark.parametrize("name,spec", [("squared", POOLS[1]), ("next_id", POOLS[1]), ("weight_on_grad", POOLS[0]),
                                       ("norm_expansion", POOLS[3])])
def test_mutants_leave_the_bound(name, spec):
    grad, emb, ids, pairs, ref, bnd = _pool(spec)
    bad = T.outside(getattr(T, "mutant_" + name)(grad, emb, ids, WEIGHT), ref, bnd)
    print(f"{name} on {spec}: {int(bad.sum())} of {bad.size} elements outside")
    assert bad.any()
    if name == "norm_expansion":
        # (the pool with an offset of 4 in every element: norms of ~34 beside distances of ~0.6) it fails where the contract
        # is exact: at v = ids[i] and at the duplicated rows
        exact = [(i, int(t)) for i, t in enumerate(ids.tolist())] + list(pairs)
        print("  of them where the contract is exact:", sum(bool(bad[i, v]) for i, v in exact), "of", len(exact))
        assert any(bad[i, v] for i, v in exact)


def test_dropping_the_embedding_scale_leaves_the_bound():
    """Gemma's case: the engine passes float32(weight * emb_scale); the mutant passes the weight alone."""
    grad, emb, ids, _, _, _ = _pool(POOLS[1])
    scale = float(torch.tensor(32 ** 0.5, dtype=torch.bfloat16))
    w_eff = T.w32(WEIGHT * scale)
    ref, bnd = T.restated64(grad, emb, ids, w_eff), T.bound(grad, emb, ids, w_eff)
    assert not T.outside(T.restated32(grad, emb, ids, w_eff), ref, bnd).any()
    assert T.outside(T.restated32(grad, emb, ids, WEIGHT), ref, bnd).any()


# ---------------------------------------------------------------------------------------------------- exact grid
@pytest.mark.parametrize("rows,V,D", [(1, 1, 8), (20, 257, 72), (33, 63, 520)])
def test_exact_grid(rows, V, D):
    grad, emb, ids, w = T.grid_pool(rows, V, D)
    for dt in T.DTYPES.values():                                  # the grid is exact in every dtype
        assert torch.equal(emb.to(dt).float(), emb) and torch.equal(grad.to(dt).float(), grad)
    ref = T.restated64(grad, emb, ids, w)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    for order in ("sequential", "pairwise"):
        assert T.restated32(grad, emb, ids, w, order).tobytes() == ref.astype(np.float32).tobytes()


# -------------------------------------------------------------------------------------------------------- options
def test_engine_option(monkeypatch):
    from bimodalattack_amd import BimodalAttackConfig
    from bimodalattack_amd.config import EngineOptions
    monkeypatch.delenv("BMA_TOKEN_DIST_WEIGHT", raising=False)
    retired = (dict(EngineOptions._RETIRED_ENV), dict(EngineOptions._RETIRED_KW))
    o = EngineOptions.from_env()
    assert o.token_dist_weight == 0.0 and EngineOptions().token_dist_weight == 0.0 and type(o.token_dist_weight) is float
    o = EngineOptions.from_env(token_dist_weight=0.25)
    assert o.token_dist_weight == 0.25 and EngineOptions.from_env().token_dist_weight == 0.0
    assert EngineOptions.from_env(token_dist_weight=2).token_dist_weight == 2.0
    monkeypatch.setenv("BMA_TOKEN_DIST_WEIGHT", "0.5")
    assert EngineOptions.from_env().token_dist_weight == 0.5
    assert EngineOptions.from_env(token_dist_weight=0.125).token_dist_weight == 0.125       # the keyword wins
    for bad in ("-1", "nan", "inf", "much", ""):
        monkeypatch.setenv("BMA_TOKEN_DIST_WEIGHT", bad)
        with pytest.raises(ValueError, match="token_dist_weight"):
            EngineOptions.from_env()
    monkeypatch.delenv("BMA_TOKEN_DIST_WEIGHT")
    for bad in (True, False, NAN, INF, -INF, -0.5, "0.1", [1.0]):
        with pytest.raises(ValueError, match="token_dist_weight"):
            EngineOptions.from_env(token_dist_weight=bad)
    # an attribute beside the dataclass fields: repr, ==, copies
    assert copy.copy(o).token_dist_weight == 0.25 and copy.deepcopy(o).token_dist_weight == 0.25
    assert repr(o).endswith("margin_kappa=0.0, token_dist_weight=0.25)") and "token_dist_weight=0.0)" in repr(EngineOptions())
    assert o != EngineOptions.from_env() and o == EngineOptions.from_env(token_dist_weight=0.25)
    assert len(dataclasses.fields(BimodalAttackConfig)) == 27 and len(dataclasses.fields(EngineOptions)) == 30
    assert "token_dist_weight" not in {f.name for f in dataclasses.fields(EngineOptions)}
    assert "never a default" in EngineOptions.__doc__ and "token_dist_weight" in EngineOptions.__doc__
    assert retired == (EngineOptions._RETIRED_ENV, EngineOptions._RETIRED_KW)
    assert len(EngineOptions._RETIRED_ENV) == 13 and len(EngineOptions._RETIRED_KW) == 12


# ------------------------------------------------------------------------------------------------ without a device
def test_entry_point_is_exported_and_validates_without_a_device():
    from bimodalattack_amd import native, ops
    from bimodalattack_amd.native import lib
    raw = ctypes.CDLL(native.LIB_PATH)
    assert hasattr(raw, "bma_token_dist_score") and "bma_token_dist_score" in native.PROTOTYPES
    assert callable(ops.token_dist_score) and ops.TOKEN_DIST_ROWS == T.R >= 32
    slot = native.KERNEL_IDS["token_dist"]
    assert lib.bma_profile_kernel_name(slot) not in (None, b"?")
    assert sorted(native.KERNEL_IDS.values()) == sorted(set(native.KERNEL_IDS.values()))      # no slot used twice
    assert lib.bma_version() == 114 == native.ABI_VERSION
    g, e, ids, out = 64, 128, 192, 256
    f = lib.bma_token_dist_score

    def call(grad=g, ld_row=100, rows=4, V=100, gdt=1, emb=e, ld_emb=8, D=8, edt=1, idp=ids, w=1.0, outp=out, ld_out=100):
        return f(grad, ld_row, rows, V, gdt, emb, ld_emb, D, edt, idp, w, outp, ld_out, None)
    for kw in (dict(rows=0), dict(rows=-1), dict(V=0), dict(D=0), dict(ld_row=99), dict(ld_out=99), dict(ld_emb=7)):
        assert call(**kw) == -1, kw
    for w in (-1.0, -1e-30, NAN, INF, -INF):
        assert call(w=w) == -1, w
    for kw in (dict(gdt=3), dict(edt=-1), dict(gdt=7, edt=7)):
        assert call(**kw) == -2, kw
    for kw in (dict(grad=None), dict(emb=None), dict(idp=None), dict(outp=None)):
        assert call(**kw) == -1, kw
    assert call(rows=65536 * T.R) == -5
    for kw in (dict(emb=e + 8), dict(D=4, ld_emb=8), dict(D=8, ld_emb=12), dict(edt=0, D=6, ld_emb=8), dict(grad=g + 1),
               dict(gdt=0, grad=g + 2), dict(outp=out + 2), dict(idp=ids + 4)):
        assert call(**kw) == -3, kw
    # the order of the checks: sizes, weight, dtypes, null pointers, alignment
    assert call(rows=0, w=-1.0, gdt=7, grad=None, emb=e + 8) == -1
    assert call(w=NAN, gdt=7, emb=e + 8) == -1 and call(gdt=7, grad=None, emb=e + 8) == -2 and call(grad=None, emb=e + 8) == -1


def test_wrapper_refuses_cpu_tensors():
    from bimodalattack_amd import ops
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        ops.token_dist_score(torch.zeros(2, 8), torch.zeros(8, 8), torch.zeros(2, dtype=torch.int64), 1.0)


# ----------------------------------------------------------- what the GPU whole-run tests rely on, on the CPU reference
KS = (4, 8, 16)
RUN_CASES = T.RUN_CASES


def test_nearest_token_sets_on_the_tiny_tables_need_no_exclusion():
    """Whole-run test (a): with a weight of 1e6 the top-k of a position is the k allowed tokens nearest its current
    token.  On the tiny models' tables (V = 256 / 264, D = 32), with 20 random current tokens, the float64 gap of
    1e6 * distance at the k boundary exceeds the two bounds for k in {4, 8, 16} at every position: no (step, position)
    pair is left out on the table's account."""
    from bimodalattack_amd import synthetic as S
    from bimodalattack_amd.utils import get_nonascii_toks
    for kind in ("opt", "llava", "gemma3"):
        model, tok, _, _ = S.tiny_case(kind)
        E = model.get_input_embeddings().weight.detach()
        V = E.shape[0]
        assert (V, E.shape[1]) == ((256, 32) if kind == "opt" else (264, 32))
        banned = get_nonascii_toks(tok).numpy()
        ids = torch.from_numpy(np.random.RandomState(3).randint(0, V, size=20))
        grad = torch.zeros(20, V)
        ref, bnd = T.restated64(grad, E, ids, 1e6), T.bound(grad, E, ids, 1e6)
        for k in KS:
            assert not T.fragile_rows(ref, bnd, k, banned, ordered=False).any(), (kind, k)


def test_nearest_token_sets_with_the_reference_gradients():
    """... and with the gradients and tokens of the CPU reference runs in the score (the engine's differ by rounding at
    step 0 and by the trajectory afterwards): the top-16 of the float64 score at weight 1e6 is the nearest-16 set at every
    (step, position) pair the tie-exclusion rule keeps, and the rule leaves out at most 5 % of them."""
    fragile, pairs = 0, 0
    for kind, mode in RUN_CASES:
        trace, E, scale, banned = _oracle_run(kind, mode)
        w_eff = T.w32(1e6 * scale)
        for st in trace:
            g, ids = st["grad_tok"][-1], st["optim_ids_in"][0]
            ref, bnd = T.restated64(g, E, ids, w_eff), T.bound(g, E, ids, w_eff)
            frag = T.fragile_rows(ref, bnd, 16, banned, ordered=False)
            near, got = T.topk64(T.distance64(E, ids), 16, banned)[0], T.topk64(ref, 16, banned)[0]
            for i in np.nonzero(~frag)[0]:
                assert set(near[i]) == set(got[i]), (kind, mode, i)
            fragile += int(frag.sum())
            pairs += frag.size
    print(f"pairs left out: {fragile} of {pairs}")
    assert fragile <= 0.05 * pairs


@functools.lru_cache(maxsize=None)
def _oracle_run(kind, mode):
    import tempfile
    from bimodalattack_amd import GCGConfig, synthetic as S
    from bimodalattack_amd.utils import get_nonascii_toks
    from oracle.attack_loop import run_oracle
    model, tok, proc, image = S.tiny_case(kind)
    cfg = GCGConfig(seed=1, verbosity="ERROR", optim_str_init=S.TINY_OPTIM_INIT, images_folder=tempfile.mkdtemp(prefix="bma_td_"),
                    **{**MODES[mode], "num_steps": 4, "topk": 16})
    _, trace, atk = run_oracle(model, tok, proc, messages_for(kind, mode), GOAL, TARGET, image if cfg.pgd_attack else None, cfg,
                               normalize=S.Normalize(S.CLIP_MEAN, S.CLIP_STD))
    E = model.get_input_embeddings().weight.detach()
    scale = getattr(model.get_input_embeddings(), "embed_scale", None)
    scale = 1.0 if scale is None else float(torch.as_tensor(scale).to(E.dtype).float())
    return trace, E, scale, get_nonascii_toks(tok).numpy()


def test_reference_alone_stays_inside_the_cap_at_the_moderate_weight():
    """Whole-run test (b), on the CPU reference (the oracle's loop, weight 0): with the weight derived from the trace, the
    float32 restatement -- the stand-in for the kernel -- picks the same top-k as float64 wherever the tie-exclusion rule
    does not apply, the rule applies to at most 5 % of the (step, position) pairs, and the top-k sets differ from the
    raw gradient's on some step (or the GPU test would show nothing)."""
    fragile, pairs, changed = 0, 0, 0
    for kind, mode in RUN_CASES:
        trace, E, scale, banned = _oracle_run(kind, mode)
        assert (scale != 1.0) == (kind == "gemma3")
        w_eff = T.w32(T.moderate_weight(trace, E, scale) * scale)
        for st in trace:
            g, ids = st["grad_tok"][-1], st["optim_ids_in"][0]
            ref, bnd = T.restated64(g, E, ids, w_eff), T.bound(g, E, ids, w_eff)
            frag = T.fragile_rows(ref, bnd, 16, banned, ordered=False)
            want = T.topk64(ref, 16, banned)[0]
            for order in ("sequential", "pairwise"):
                got = T.topk64(T.restated32(g, E, ids, w_eff, order).astype(np.float64), 16, banned)[0]
                for i in np.nonzero(~frag)[0]:
                    assert set(got[i]) == set(want[i]), (kind, mode, order, i)
            raw = T.topk64(np.asarray(g, np.float64), 16, banned)[0]
            changed += any(set(a) != set(b) for a, b in zip(raw, want))
            fragile += int(frag.sum())
            pairs += frag.size
    assert pairs >= 5 * 4 * 8 and fragile <= 0.05 * pairs, (fragile, pairs)
    assert changed >= 1
