"""The Carlini-Wagner margin target loss on the MI355X: bma_margin_target against the float64 restatement of the contract
(margin_ref.py) through `ops` and once through the raw C ABI, and whole runs with ``loss_rule="margin"`` on the tiny
synthetic models against a recomputation in the test (plain fp32 HF forward on the CPU, then the float64 rule).

What is compared how: the row margins m, the runner-up index i, match and dlogits are exact by contract (one fp32
subtraction of two representable values, comparisons, and dtype(+-g)), so they are compared bit for bit.  The loss is
exact on the eighths grid (every partial sum is representable) and compared bit for bit there; on generic inputs it is
held to (T + 2) * 2^-24 * mean_j |l_j| of float64 -- one rounding per subtraction, T - 1 in the sum, one in the division."""

import functools
import os
import tempfile

import numpy as np
import pytest
import torch

import margin_ref as R
import test_mellowmax_gpu as MG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
INF, NAN = float("inf"), float("nan")
KAPPA_GRID = 0.25                      # exact on the grid: margins of exactly -kappa occur


def bits(x):
    return x.detach().contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32).cpu().numpy()


def same_f32(got: torch.Tensor, want: np.ndarray) -> bool:
    """float32 values equal bit for bit, any NaN standing for any NaN."""
    g, w = got.detach().float().cpu().numpy().reshape(-1), np.asarray(want, np.float32).reshape(-1)
    return bool(np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~np.isnan(w)].view(np.int32), w[~np.isnan(w)].view(np.int32)))


def labels_at(T, V):
    """Seeded labels with the placements that matter: 0 and V - 1 (first and last row), one element in (the head of a row
    that starts off the 16-byte grid), V - 2 (its tail) and the middle (a vector)."""
    lab = R.labels_for(T, V)
    for j, v in ((1, 1), (2, V - 2), (3, V // 2)):
        if T > j + 1:
            lab[j] = min(max(v, 0), V - 1)
    return lab


def plant(z, lab, kappa):
    """Rows of the grid pool rewritten by (b * T + j) % 5: 1 = the label is the row maximum; 2 = the label ties with the
    runner-up; 3 = the runner-up sits next to the label (lab ^ 1: the same 16-byte vector wherever the row's vectors
    start on an even element, which V odd and the off-grid layouts vary); 4 = the margin is exactly -kappa."""
    B, T, V = z.shape
    for b in range(B):
        for j in range(T):
            y, kind = int(lab[j]), (b * T + j) % 5
            others = np.delete(z[b, j], y)
            if kind == 1:
                z[b, j, y] = 20.0
            elif kind == 2:
                z[b, j, y] = others.max()
            elif kind == 3:
                z[b, j, (y ^ 1) if (y ^ 1) < V else y - 1] = 18.0
            elif kind == 4:
                z[b, j, y] = others.max() + kappa
    return z


def layouts(x):
    """The same (B, T, V) values as a contiguous tensor; as a view with ld_row = V + 3 and a candidate stride that is not
    T * ld_row; starting one element off the 16-byte grid; and with a last stride that is not 1 (the wrapper's
    .contiguous() fallback)."""
    B, T, V = x.shape
    big = torch.full((B, T + 2, V + 3), 30.0, dtype=x.dtype, device=x.device)      # (30: above every logit if ever read)
    big[:, 1:T + 1, :V] = x
    flat = torch.full((B * T * V + 9,), 30.0, dtype=x.dtype, device=x.device)
    off = 1                                                                      # one element past a boundary
    flat[off:off + B * T * V] = x.reshape(-1)
    shifted = flat[off:off + B * T * V].view(B, T, V)
    assert shifted.data_ptr() % 16 == x.element_size()
    turned = x.transpose(1, 2).contiguous().transpose(1, 2)
    assert turned.stride(2) != 1 or V == 1 or T == 1
    return dict(contiguous=x.contiguous(), padded=big[:, 1:T + 1, :V], shifted=shifted, turned=turned)


def check_call(x, lab, labd, kappa, ref, grid, gs=0.375):
    from bimodalattack_amd import ops
    B, T, V = x.shape
    loss, match, dlog, m = ops.margin_target(x, labd, kappa, want_match=True, want_dlogits=True, grad_scale=gs)
    assert loss.dtype == torch.float32 and m.shape == (B, T) and match.dtype == torch.int32 and dlog.dtype == x.dtype
    assert same_f32(m, ref["m"]), "m"
    assert np.array_equal(match.cpu().numpy() != 0, ref["match"]), "match"
    assert torch.equal(match, ops.ce_target(x, labd, want_match=True)[1]), "match against ce_target's"
    want_d = torch.from_numpy(ref["dlogits"].astype(np.float32)).to(x.dtype)
    assert np.array_equal(bits(dlog), bits(want_d)), "dlogits"
    if grid:
        assert same_f32(loss, R.expected_loss32(ref)), "loss"
    else:
        fin = np.isfinite(ref["loss"])
        assert same_f32(loss[torch.from_numpy(~fin).to(loss.device)], ref["loss"][~fin]), "loss, special values"
        with np.errstate(invalid="ignore"):                                      # (the special values, masked out right away)
            err, bound = np.abs(loss.double().cpu().numpy() - ref["loss"])[fin], R.loss_bound(ref, T, kappa)[fin]
        print(f"B={B} T={T} V={V} {x.dtype}: worst loss error {err.max(initial=0.0):.3e}, its bound {bound.max(initial=0.0):.3e}")
        assert (err <= bound).all(), (err, bound)
    return loss, match, dlog, m


# ------------------------------------------------------------------ the kernels against the restatement
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("V", [2, 7, 257, 1000, 2049])
@pytest.mark.parametrize("T", [1, 5, 20, 65])
def test_kernel_equals_the_restatement(T, V, dt):
    dtype, lab, kappa = DTYPES[dt], labels_at(T, V), KAPPA_GRID
    labd = torch.from_numpy(lab).to(DEV)
    for B in (1, 5):
        z = plant(R.grid_pool(B, T, V), lab, kappa)
        x = torch.from_numpy(z).to(DEV, dtype)
        assert torch.equal(x.float().cpu(), torch.from_numpy(z))                 # the grid is exact in every dtype
        ref = R.restated64(z, lab, kappa, grad_scale=0.375)
        for name, view in layouts(x).items():
            check_call(view, lab, labd, kappa, ref, grid=True)
        # generic values: the same exact outputs, the loss within its rounding bound
        xg = torch.from_numpy(R.generic_pool(B, T, V)).to(DEV, dtype)
        refg = R.restated64(xg.float().cpu().numpy(), lab, kappa, grad_scale=0.375)
        check_call(xg, lab, labd, kappa, refg, grid=False)
        check_call(layouts(xg)["shifted"], lab, labd, kappa, refg, grid=False)


def test_large_vocabulary():
    """Gemma-3's vocabulary: 32,776 vectors per row, every lane's loop past its first trip, ties throughout."""
    B, T, V, kappa = 2, 3, 262208, KAPPA_GRID
    lab = np.array([0, V // 2 + 3, V - 1])
    z = plant(R.grid_pool(B, T, V), lab, kappa)
    x = torch.from_numpy(z).to(DEV, torch.bfloat16)
    ref = R.restated64(z, lab, kappa, grad_scale=0.375)
    assert (ref["i"] > 0).all() and ref["a"].any()
    labd = torch.from_numpy(lab).to(DEV)
    check_call(x, lab, labd, kappa, ref, grid=True)
    check_call(layouts(x)["shifted"], lab, labd, kappa, ref, grid=True)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("kappa", [0.0, 0.05, INF])
def test_special_values_and_kappa(kappa, dt):
    """NaN off and at the label, a label of -inf, a row of -inf, every v != y NaN, a label outside [0, V); kappa = 0, a
    kappa that float32 rounds, and +inf (no clamp)."""
    dtype, T, V = DTYPES[dt], 6, 1000
    k32 = float(np.float32(kappa))                              # the launch argument is a float
    lab = labels_at(T, V)
    z = plant(R.grid_pool(6, T, V, seed=1), lab, 0.25)
    z[0, 1, 517] = NAN
    z[1, 2, lab[2]] = NAN
    z[2, 3, lab[3]] = -INF
    z[3, 0, :] = -INF
    z[4, 4, :] = NAN
    z[4, 4, lab[4]] = 1.0
    z[5, 5, 3] = INF
    x, labd = torch.from_numpy(z).to(DEV, dtype), torch.from_numpy(lab).to(DEV)
    ref = R.restated64(z, lab, k32, grad_scale=0.375)
    assert np.array_equal(np.isnan(ref["loss"]), [True, True, False, True, True, False]) and ref["loss"][2] == INF
    assert ref["i"][4, 4] == -1 and ref["loss"][5] == INF
    # (kappa = 0.05 is no eighth: sums of clamped and free rows round, so that loss is held to the bound)
    for view in layouts(x).values():
        check_call(view, lab, labd, k32, ref, grid=kappa != 0.05)
    bad = lab.copy()
    bad[2] = V
    ref = R.restated64(z, bad, k32, grad_scale=0.375)
    assert np.isnan(ref["loss"]).all() and not ref["match"].any() and (ref["dlogits"][:, 2] == 0).all()
    from bimodalattack_amd import ops
    loss, match, dlog, m = ops.margin_target(x, torch.from_numpy(bad).to(DEV), k32, want_match=True, want_dlogits=True, grad_scale=0.375)
    assert torch.isnan(loss).all() and same_f32(m, ref["m"]) and not match.any()
    assert np.array_equal(bits(dlog), bits(torch.from_numpy(ref["dlogits"].astype(np.float32)).to(dtype)))
    bad[2] = -1
    assert torch.isnan(ops.margin_target(x, torch.from_numpy(bad).to(DEV), k32)[0]).all()


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_two_calls_out_tensor_and_guards(dt):
    """Two calls are bitwise equal; `out=` takes dlogits at any element-aligned start and nothing around it is touched."""
    from bimodalattack_amd import ops
    dtype, (B, T, V), kappa = DTYPES[dt], (3, 5, 1003), KAPPA_GRID
    lab = labels_at(T, V)
    z = plant(R.grid_pool(B, T, V), lab, kappa)
    x, labd = torch.from_numpy(z).to(DEV, dtype), torch.from_numpy(lab).to(DEV)
    ref = R.restated64(z, lab, kappa, grad_scale=2.0)
    want_d = bits(torch.from_numpy(ref["dlogits"].astype(np.float32)).to(dtype))
    n, guard = B * T * V, 64
    for offset in (0, 1, 3):
        outs = []
        for _ in range(2):
            flat = torch.full((guard + offset + n + guard,), 7.0, dtype=dtype, device=DEV)
            out = flat[guard + offset:guard + offset + n].view(B, T, V)
            loss, match, dlog, m = ops.margin_target(x, labd, kappa, want_match=True, want_dlogits=True, grad_scale=2.0, out=out)
            assert dlog.data_ptr() == out.data_ptr()
            assert (flat[:guard + offset] == 7.0).all() and (flat[guard + offset + n:] == 7.0).all()
            outs.append((loss, match, dlog, m))
        for a, b in zip(*outs):
            assert np.array_equal(bits(a), bits(b))
        assert np.array_equal(bits(outs[0][2]), want_d)
    loss, match, dlog, m = ops.margin_target(x, labd, kappa)
    assert match is None and dlog is None and same_f32(loss, R.expected_loss32(ref))


def test_raw_c_abi():
    """bma_margin_target itself: ld_row = V + 3, a start off the 16-byte grid, and the whole scratch (m | i | row hit)."""
    from bimodalattack_amd import native, ops
    (B, T, V), kappa, dtype = (5, 20, 1000), KAPPA_GRID, torch.bfloat16
    lab = labels_at(T, V)
    z = plant(R.grid_pool(B, T, V), lab, kappa)
    ref = R.restated64(z, lab, kappa, grad_scale=1.0)
    ld_row, ld_cand = V + 3, (T + 1) * (V + 3)
    store = torch.full((B * ld_cand + 9,), 30.0, dtype=dtype, device=DEV)
    start = 1
    block = store[start:start + B * ld_cand].view(B, T + 1, ld_row)
    block[:, :T, :V] = torch.from_numpy(z).to(DEV, dtype)
    assert block.data_ptr() % 16 == 2
    labd = torch.from_numpy(lab).to(DEV)
    ws = torch.full((3 * B * T + 1,), -7, dtype=torch.int32, device=DEV)
    loss, match = torch.empty(B, dtype=torch.float32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
    dlog = torch.full((B * T * V + 1,), 7.0, dtype=dtype, device=DEV)
    assert native.lib.bma_margin_target_ws_bytes(B, T) == 3 * B * T * 4
    rc = native.lib.bma_margin_target(block.data_ptr(), ld_cand, ld_row, labd.data_ptr(), B, T, V, 1, kappa, ws.data_ptr(),
                                      loss.data_ptr(), match.data_ptr(), dlog.data_ptr(), 1.0, ops._stream(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    BT = B * T
    assert same_f32(ws[:BT].view(torch.float32), ref["m"])
    assert np.array_equal(ws[BT:2 * BT].cpu().numpy().reshape(B, T), ref["i"])
    z64 = z.astype(np.float64)
    row_hit = (z64.argmax(-1) == lab[None])                                      # numpy's argmax: the first maximum
    assert np.array_equal(ws[2 * BT:3 * BT].cpu().numpy().reshape(B, T), row_hit.astype(np.int32))
    assert int(ws[3 * BT]) == -7 and float(dlog[-1]) == 7.0
    assert same_f32(loss, R.expected_loss32(ref)) and np.array_equal(match.cpu().numpy() != 0, ref["match"])
    assert np.array_equal(bits(dlog[:-1].view(B, T, V)), bits(torch.from_numpy(ref["dlogits"].astype(np.float32)).to(dtype)))


def test_autograd_function_matches_torch_autograd():
    from bimodalattack_amd import ops
    T, V, kappa = 20, 1003, 0.5
    lab = labels_at(T, V)
    rs = np.random.RandomState(5)
    z = np.stack([rs.permutation(V) / 8.0 - 60.0 for _ in range(T)]).astype(np.float32)      # no ties: torch's max is unambiguous
    z[3, lab[3]] = 100.0                                                                       # a won row: no gradient
    x = torch.from_numpy(z).to(DEV).requires_grad_()
    loss = ops.TargetMargin.apply(x, torch.from_numpy(lab).to(DEV), kappa)
    (3.0 * loss).backward()
    want, g64 = R.autograd64(z[None], lab, kappa, grad_scale=3.0)
    assert float(loss) == float(np.float32(want[0]))
    g = x.grad.cpu().double().numpy()
    assert np.array_equal(g != 0, g64[0] != 0) and (g[3] == 0).all()
    np.testing.assert_allclose(g, g64[0], rtol=2 ** -22, atol=0)                 # g = fl(1/T), times 3: two roundings


def test_wrapper_checks():
    from bimodalattack_amd import ops
    x, lab = torch.zeros(2, 3, 8, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV)
    for bad in (-1.0, -INF, NAN):
        with pytest.raises(ValueError, match="kappa"):
            ops.margin_target(x, lab, bad)
    with pytest.raises(ValueError):
        ops.margin_target(x[:, :, :1], lab, 0.0)                                 # V = 1: no wrong logit
    with pytest.raises(ValueError):
        ops.margin_target(x, lab, 0.0, want_dlogits=True, out=torch.zeros(2, 3, 8, device=DEV, dtype=torch.float16))
    with pytest.raises(ValueError):
        ops.margin_target(x, lab[:2], 0.0)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        ops.margin_target(x.cpu(), lab.cpu(), 0.0)
    loss, match, dlog, m = ops.margin_target(x[:0], lab, 0.0, want_match=True)
    assert loss.shape == (0,) and match.shape == (0,) and m.shape == (0, 3)


# ------------------------------------------------------------------ whole runs
GOAL, TARGET, KAPPA, loss_tol = R.GOAL, R.TARGET, R.RUN_KAPPA, R.loss_tol


def run_margin(kind, mode, steps=4, cfg_over=None, trace=True, target=TARGET, **engine):
    from bimodalattack_amd import run, synthetic as S
    model, tok, proc, image = S.tiny_case(kind, device=DEV)
    cfg = R.run_config(mode, steps, **(cfg_over or {}))
    tr = [] if trace else None
    engine.setdefault("loss_rule", "margin")
    engine.setdefault("margin_kappa", KAPPA)
    res = run(model, tok, proc, R.messages_for(kind, mode), GOAL, target, image, cfg, normalize=S.Normalize(S.CLIP_MEAN, S.CLIP_STD),
              rng_device="cpu", trace=tr, strict=True, save_images=False, **engine)
    return res, tr, cfg


class _Recompute(MG._Recompute):
    """The mellowmax test's recomputation (the tiny model on the CPU in fp32 through its plain HF forward) with the
    float64 margin as the rule, and the tolerance's scale taken from the label AND the runner-up logits."""

    def _rows(self, embeds):
        self.rows = super()._rows(embeds)
        return self.rows

    def _loss(self, rows):
        return R.torch_margin(rows.double(), self.labels, KAPPA)

    def scores(self, ids, image, final=False):
        loss, _, hit = super().scores(ids, image, final)
        return loss, R.row_facts(self.rows, self.labels, KAPPA)[2], hit


@functools.lru_cache(maxsize=None)
def _compared(kind, mode):
    """One traced run of the engine held to the recomputation, step by step; returns, per step with candidates, whether
    the winner comparison was skipped as a near-tie (top two recomputed losses within the tolerance)."""
    res, trace, cfg = run_margin(kind, mode)
    rc = _Recompute(kind, mode, cfg)
    assert len(trace) == cfg.num_steps == len(res.losses)
    image = rc.image0.numpy()
    ties = []
    for i, st in enumerate(trace):
        if i == 0:
            # the gradients of step 0 against torch autograd of the restated loss through the same model (the site is not
            # fragile in the reference: test_margin.py)
            g_tok, g_img = rc.gradients(st["optim_ids_in"], image)
            if g_tok is not None:
                np.testing.assert_allclose(st["grad_tok"][0], g_tok, rtol=2e-3, atol=1e-4 * float(np.abs(g_tok).max()))
            if g_img is not None:
                np.testing.assert_allclose(st["grad_img"][0], g_img, rtol=5e-3, atol=1e-4 * float(np.abs(g_img).max()))
        if cfg.pgd_attack:
            image = st["image_after_pgd"]
        ids = st.get("filtered", st.get("sampled")) if cfg.gcg_attack else st["optim_ids_in"]
        want, scale, _ = rc.scores(ids, image)
        tol = loss_tol(scale)
        got = st["losses"][0]
        assert got.shape == want.shape
        print(f"{kind}/{mode} step {i}: worst candidate loss error {np.abs(got - want).max():.3e} (tolerance {tol:.3e})")
        np.testing.assert_allclose(got, want, rtol=0, atol=tol, err_msg=f"step {i}")
        if cfg.gcg_attack and cfg.pgd_attack:
            b = st["best_idx"]
            final = rc.scores(ids[b:b + 1], image, final=True)[0][0]
        else:
            final = want.min()
        np.testing.assert_allclose(res.losses[i], final, rtol=0, atol=tol)
        if cfg.gcg_attack:
            two = np.sort(want)[:2]
            tie = bool(len(two) > 1 and two[1] - two[0] <= tol)
            ties.append(tie)
            if not tie:
                assert st["best_idx"] == int(want.argmin()), f"step {i}: winner"
    return tuple(ties)


@pytest.mark.parametrize("kind,mode", R.CASES)
def test_run_equals_the_recomputation(kind, mode):
    _compared(kind, mode)


def test_near_tie_share():
    """At most 5 % of the steps compared may be skipped as near-ties, over all cases (made here if not made yet)."""
    ties = [t for kind, mode in R.CASES for t in _compared(kind, mode)]
    assert len(ties) == 16 and np.mean(ties) <= 0.05, (sum(ties), len(ties))


@pytest.mark.parametrize("engine", [dict(graph_gradient=False, graph_scoring=False), dict(ragged_suffix=False),
                                    dict(shared_prefix_attention=False), dict(gradient_ahead=False)])
def test_routes_agree(engine):
    """Graphs on and off, the ragged and the shared-prefix forward on and off: the same rule, the same losses."""
    for mode in ("joint", "gcg"):
        base, _, _ = _base_run(mode)
        res, _, _ = run_margin("llava", mode, trace=False, **engine)
        np.testing.assert_allclose(res.losses, base.losses, rtol=0, atol=1e-4)
        assert res.strings == base.strings


@functools.lru_cache(maxsize=None)
def _base_run(mode):
    return run_margin("llava", mode, trace=False)


def test_early_stop_comes_from_the_margin_pass(monkeypatch):
    """early_stop under the rule: the run ends at the first step one of whose candidates has argmax(row) == label on
    every target row (recomputed here), not before and not later -- and the cross-entropy kernel is never called: the hit
    comes out of the margin's own read of the logits."""
    from bimodalattack_amd import ops

    def refuse(*a, **k):
        raise AssertionError("loss_rule='margin' called ops.ce_target")
    monkeypatch.setattr(ops, "ce_target", refuse)
    E = R.EARLY
    res, trace, cfg = run_margin(E["kind"], E["mode"], steps=E["steps"], cfg_over=dict(early_stop=True), target=E["target"])
    rc = _Recompute(E["kind"], E["mode"], cfg, E["target"])
    first = None
    for i, st in enumerate(trace):
        want, scale, hit = rc.scores(st.get("filtered", st.get("sampled")), None)
        np.testing.assert_allclose(st["losses"][0], want, rtol=0, atol=loss_tol(scale))
        if hit.any():
            first = i
            break
    assert first is not None and first < cfg.num_steps - 1, first
    assert len(trace) == first + 1 == len(res.losses)
    assert res.losses[-1] == float(np.float32(-KAPPA))                           # T = 1: the won row, clamped


def test_default_rule_is_unchanged():
    """loss_rule left alone, and "ce" given explicitly (a kappa beside it is unread): the golden trajectory of the default
    rule (g5_llava_gcg), as before."""
    import json
    from bimodalattack_amd import BimodalAttackConfig, run, synthetic as S
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    m = json.load(open(os.path.join(golden, "g5_meta.json")))["cases"]["llava_gcg"]
    z = np.load(os.path.join(golden, "g5_llava_gcg.npz"))
    out = []
    for rule, kappa in ((None, None), ("ce", 0.5)):
        model, tok, proc, image = S.tiny_case(m["kind"], device=DEV)
        cfg = BimodalAttackConfig(seed=1, verbosity="ERROR", optim_str_init=m["optim_str_init"], images_folder=tempfile.mkdtemp(),
                                  **m["config"])
        out.append(run(model, tok, proc, m["goal"], m["goal"], m["target"], image, cfg, normalize=S.Normalize(S.CLIP_MEAN, S.CLIP_STD),
                       rng_device="cpu", strict=True, loss_rule=rule, margin_kappa=kappa))
    assert out[0].losses == out[1].losses and out[0].strings == out[1].strings
    np.testing.assert_allclose(out[0].losses, z["losses"], rtol=1e-4)
    assert out[0].strings == m["strings"]


def test_engine_keeps_the_kappa_it_was_given():
    """The options object reaches the engine as from_env made it: rule and kappa are attributes, not dataclass fields, and
    must not be lost on the way."""
    from bimodalattack_amd import synthetic as S
    from bimodalattack_amd.attack import BimodalAttack
    from bimodalattack_amd.config import EngineOptions
    model, tok, proc, image = S.tiny_case("llava", device=DEV)
    atk = BimodalAttack(model, tok, proc, R.run_config("gcg", 1), None,
                        EngineOptions.from_env(loss_rule="margin", margin_kappa=0.125, save_images=False))
    assert atk.opt.loss_rule == "margin" and atk.opt.margin_kappa == 0.125 and atk._margin_kappa == 0.125 and atk._mm_alpha is None
    atk = BimodalAttack(model, tok, proc, R.run_config("gcg", 1), None, EngineOptions.from_env(margin_kappa=0.125, save_images=False))
    assert atk.opt.loss_rule == "ce" and atk._margin_kappa is None


@pytest.mark.parametrize("mode", ["gcg", "joint", "pgd"])
def test_no_host_reads_added(mode):
    from test_apgd_gpu import _HostReads
    counts = {}
    for rule in ("ce", "margin"):
        run_margin("llava", mode, steps=2, trace=False, loss_rule=rule, filter_first=False)       # warm
        with _HostReads() as h:
            run_margin("llava", mode, steps=6, trace=False, loss_rule=rule, filter_first=False)
        counts[rule] = h.n
    assert counts["margin"] == counts["ce"], counts
