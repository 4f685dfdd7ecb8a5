"""The mellowmax target loss on the MI355X: bma_mellowmax_target against the float64 restatement and the reference's own
outputs (mellowmax_ref.py, tests/golden/g9_mellowmax_unit.npz), and whole runs with ``loss_rule="mellowmax"`` on the tiny
synthetic models against a recomputation in the test (plain fp32 HF forward on the CPU, then the float64 rule).

Tolerance of the kernel (mellowmax_ref.bounds): 4 x the largest error of the fp32 torch evaluation of the reference's
function against float64 over the (T, alpha) class's inputs, plus one rounding of the output dtype for dlogits; special
values are compared exactly."""

import functools
import os
import tempfile

import numpy as np
import pytest
import torch

import mellowmax_ref as R
from test_mellowmax import golden_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def labels_for(T, V, seed=0):
    lab = np.random.RandomState(seed + 7 * T + V).randint(0, V, size=T).astype(np.int64)
    lab[0], lab[-1] = 0, V - 1                                   # (T = 1: V - 1)
    return lab


def planted(t, labels, V, dtype, pad_rows=0, pad_cols=0, seed=0):
    """(B, T, V) device logits of `dtype` whose label columns hold -t (eighths: exact in every dtype), as a view of a
    (B, T + pad_rows, V + pad_cols) block: ld_row > V, and a candidate stride that is not T * ld_row."""
    B, T = t.shape
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    big = (torch.randint(-128, 128, (B, T + pad_rows, V + pad_cols), device=DEV, generator=g).to(torch.float32) / 8).to(dtype)
    view = big[:, pad_rows // 2:pad_rows // 2 + T, :V]
    j = torch.arange(T, device=DEV)
    view[:, j, torch.from_numpy(labels).to(DEV)] = (-torch.from_numpy(t)).to(DEV, dtype)
    return view


def as_f64(x):
    return x.detach().to(torch.float32).cpu().numpy().astype(np.float64)


def bits(x):
    return x.detach().contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32)


# ------------------------------------------------------------------ the loss pass
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("V", [17, 4099, 32064])
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 257, 1025])
def test_loss_and_weights_at_every_shape(T, V, dt):
    from bimodalattack_amd import ops
    dtype, pool, lab = DTYPES[dt], R.pool(T), labels_for(T, V)
    labd = torch.from_numpy(lab).to(DEV)
    worst = 0.0
    for B in (1, 3):
        t = pool[:B]
        strided = planted(t, lab, V, dtype, pad_rows=2, pad_cols=5)
        assert strided.stride(1) > V and strided.stride(0) != T * strided.stride(1)
        for x in (strided, strided.contiguous()):
            for alpha in R.ALPHAS:
                lb, wb = R.bounds(pool, alpha, key=(T, alpha))
                l64, w64 = R.restated64(t, alpha)
                loss, match, dlog, w = ops.mellowmax_target(x, labd, alpha)
                assert match is None and dlog is None and loss.dtype == torch.float32 and w.shape == (B, T)
                el, ew = np.abs(as_f64(loss) - l64).max(), np.abs(as_f64(w) - w64).max()
                worst = max(worst, el / lb if lb else el)
                assert el <= lb and ew <= wb, (B, alpha, el, lb, ew, wb)
    print(f"T={T} V={V} {dt}: worst loss error / bound = {worst:.3f}")


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 257, 1025])
def test_every_pool_row(T):
    """All rows the bounds were measured on go through the kernel (B = 64: sixteen workgroups of the wave-per-candidate
    route, 64 of the workgroup-per-candidate one)."""
    from bimodalattack_amd import ops
    pool, lab = R.pool(T), labels_for(T, 17)
    x = planted(pool, lab, 17, torch.float32)
    for alpha in R.ALPHAS:
        lb, wb = R.bounds(pool, alpha, key=(T, alpha))
        l64, w64 = R.restated64(pool, alpha)
        loss, _, _, w = ops.mellowmax_target(x, torch.from_numpy(lab).to(DEV), alpha)
        el, ew = np.abs(as_f64(loss) - l64).max(), np.abs(as_f64(w) - w64).max()
        print(f"T={T} alpha={alpha}: loss error {el:.3e} (bound {lb:.3e}), w error {ew:.3e} (bound {wb:.3e})")
        assert el <= lb and ew <= wb, (alpha, el, lb, ew, wb)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_golden_rows_and_special_values(dt):
    """The reference's own outputs: finite rows within 4 x the reference's fp32 error on them, special rows exactly (NaN,
    +inf, -inf), in the loss, the weights and dlogits; a NaN off the label columns is never read."""
    from bimodalattack_amd import ops
    dtype = DTYPES[dt]
    for T, alpha, logits, labels, o32, o64 in golden_cases():
        x, lab = torch.from_numpy(logits).to(DEV, dtype), torch.from_numpy(labels).to(DEV)
        loss, _, dlog, w = ops.mellowmax_target(x, lab, alpha, want_dlogits=True, grad_scale=2.0)
        got = as_f64(loss)
        assert R.same_special(got, o64), (T, alpha, got, o64)
        ok = np.isfinite(o64)
        bound = 4.0 * np.abs(o32[ok].astype(np.float64) - o64[ok]).max()
        err = np.abs(got[ok] - o64[ok]).max()
        assert err <= bound, (T, alpha, err, bound)
        t = R.gather_t(logits, labels)
        g64 = R.autograd64(t, alpha)[1]
        wb = R.bounds(t, alpha)[1]
        wg = as_f64(w)
        assert np.array_equal(np.isnan(wg), np.isnan(g64)), (T, alpha)
        fin = ~np.isnan(g64)
        assert np.abs(wg[fin] - g64[fin]).max() <= wb, (T, alpha)
        d = as_f64(dlog)
        at = np.zeros(d.shape, bool)
        at[:, np.arange(T), labels] = True
        assert (d[~at] == 0).all()
        dl = d[:, np.arange(T), labels]
        assert np.array_equal(np.isnan(dl), np.isnan(g64))
        assert (np.abs(dl[fin] + 2.0 * g64[fin]) <= 2.0 * wb + R.ulp(2.0 * g64[fin], dtype)).all(), (T, alpha)


# ------------------------------------------------------------------ the dlogits pass
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("B,T,V", [(1, 20, 4099), (3, 2, 17)])
def test_dlogits_every_element(B, T, V, dt, offset):
    """Zeros and label entries element by element, in a block that starts `offset` elements off the allocation (rows of
    4099 or 17 elements start on every residue of the 16-byte grid either way), grad_scale != 1, guard elements around the
    block untouched, and two calls bitwise equal."""
    from bimodalattack_amd import ops
    dtype, alpha, gs = DTYPES[dt], 1.0, 0.375
    pool, lab = R.pool(T), labels_for(T, V)
    t = pool[:B]
    x, labd = planted(t, lab, V, dtype), torch.from_numpy(lab).to(DEV)
    n, guard = B * T * V, 64
    outs = []
    for _ in range(2):
        flat = torch.full((guard + offset + n + guard,), 7.0, dtype=dtype, device=DEV)
        out = flat[guard + offset:guard + offset + n].view(B, T, V)
        loss, _, dlog, w = ops.mellowmax_target(x, labd, alpha, want_dlogits=True, grad_scale=gs, out=out)
        assert dlog.data_ptr() == out.data_ptr() and (out.data_ptr() % 16 != 0 or offset == 0)
        assert (flat[:guard + offset] == 7.0).all() and (flat[guard + offset + n:] == 7.0).all()
        outs.append((loss, w, dlog))
    for a, b in zip(*outs):
        assert torch.equal(bits(a), bits(b))
    wb = R.bounds(pool, alpha, key=(T, alpha))[1]
    w64 = R.restated64(t, alpha)[1]
    d = as_f64(outs[0][2])
    at = np.zeros(d.shape, bool)
    at[:, np.arange(T), lab] = True
    assert (d[~at] == 0).all()
    want = -w64 * gs
    err = np.abs(d[:, np.arange(T), lab] - want)
    assert (err <= wb * gs + R.ulp(want, dtype)).all(), (err.max(), wb)


def test_autograd_function_matches_torch_autograd():
    from bimodalattack_amd import ops
    T, V, alpha = 20, 4099, 4.0
    pool, lab = R.pool(T), labels_for(T, V)
    x = planted(pool[:1], lab, V, torch.float32)[0].clone().requires_grad_()
    labd = torch.from_numpy(lab).to(DEV)
    loss = ops.TargetMellowmax.apply(x, labd, alpha)
    (3.0 * loss).backward()
    x64 = x.detach().cpu().double().requires_grad_()
    want = R.torch_mellowmax(-x64[torch.arange(T), torch.from_numpy(lab)], alpha)
    (3.0 * want).backward()
    lb, wb = R.bounds(pool, alpha, key=(T, alpha))
    assert abs(float(loss) - float(want)) <= lb
    g, g64 = x.grad.cpu().double().numpy(), x64.grad.numpy()
    assert (g[g64 == 0] == 0).all()
    assert (np.abs(g - g64) <= 3.0 * wb + R.ulp(g64, torch.float32) + (g64 == 0)).all()


def test_wrapper_checks():
    from bimodalattack_amd import ops
    x, lab = torch.zeros(2, 3, 8, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            ops.mellowmax_target(x, lab, bad)
    with pytest.raises(ValueError):
        ops.mellowmax_target(x, lab, 1.0, want_dlogits=True, out=torch.zeros(2, 3, 8, device=DEV, dtype=torch.float16))
    loss, _, _, w = ops.mellowmax_target(x[:0], lab, 1.0)
    assert loss.shape == (0,) and w.shape == (0, 3)
    # a label outside [0, V) is never read through: the candidate is NaN, like ce_target's
    loss, _, dlog, w = ops.mellowmax_target(x, torch.tensor([1, 8, 2], device=DEV), 1.0, want_dlogits=True)
    assert torch.isnan(loss).all() and torch.isnan(w).all() and (dlog[:, 1] == 0).all()


# ------------------------------------------------------------------ whole runs
GOAL, TARGET, MODES, ALPHA, loss_tol = R.GOAL, R.TARGET, R.MODES, R.RUN_ALPHA, R.loss_tol


def run_mm(kind, mode, steps=4, cfg_over=None, trace=True, target=TARGET, **engine):
    from bimodalattack_amd import run, synthetic as S
    model, tok, proc, image = S.tiny_case(kind, device=DEV)
    cfg = R.run_config(mode, steps, **(cfg_over or {}))
    tr = [] if trace else None
    engine.setdefault("loss_rule", "mellowmax")
    res = run(model, tok, proc, R.messages_for(kind, mode), GOAL, target, image, cfg, normalize=S.Normalize(S.CLIP_MEAN, S.CLIP_STD),
              rng_device="cpu", trace=tr, strict=True, save_images=False, **engine)
    return res, tr, cfg


class _Recompute:
    """The test's own evaluation: the tiny model on the CPU in fp32 through its plain HF forward (the oracle's prompt
    segments and splice, nothing of the engine), then the float64 rule."""

    def __init__(self, kind, mode, cfg, target=TARGET):
        from bimodalattack_amd import synthetic as S
        from oracle.attack_loop import OracleAttack
        self.model, tok, proc, self.image0 = S.tiny_case(kind, device="cpu")
        self.o = OracleAttack(self.model, tok, proc, cfg, S.Normalize(S.CLIP_MEAN, S.CLIP_STD))
        self.o._prepare(R.messages_for(kind, mode), target)
        self.cfg, self.T = cfg, self.o.target_ids.shape[1]
        self.labels = self.o.target_ids[0]

    def _rows(self, embeds):
        logits = self.model(inputs_embeds=embeds).logits
        return logits[:, embeds.shape[1] - self.T - 1:-1, :]

    def _loss(self, rows):
        return R.torch_mellowmax(-rows.double()[:, torch.arange(self.T), self.labels], ALPHA)

    def scores(self, ids, image, final=False):
        """(losses float64 (n,), max |target logit|, early-stop hits) of the candidates as the step scored them; final: of
        the step's winner as the step re-scores it with the image."""
        cfg, o = self.cfg, self.o
        ids = torch.from_numpy(np.asarray(ids))
        with torch.no_grad():
            if cfg.pgd_attack:
                feats = o._image_features(torch.from_numpy(image))
                if cfg.gcg_attack and not final:
                    emb = o._splice(ids, feats, ids.shape[0], "pgd", single=True)
                else:
                    emb = o._splice(ids, feats, None, "gcg_pgd")
            else:
                emb = o._splice(ids, None, ids.shape[0], "gcg", no_joint_eval=True)
            rows = self._rows(emb)
            hit = (rows.argmax(-1) == self.labels).all(-1)
            tl = rows[:, torch.arange(self.T), self.labels]
            return self._loss(rows).numpy(), float(tl.abs().max()), hit.numpy()

    def gradients(self, optim_ids, image):
        cfg, o = self.cfg, self.o
        V = o.emb.num_embeddings
        onehot = torch.nn.functional.one_hot(torch.from_numpy(optim_ids), num_classes=V).to(torch.float32).requires_grad_()
        optim = onehot @ o.emb.weight
        img = None
        if cfg.pgd_attack:
            img = torch.from_numpy(image).clone().requires_grad_()
            parts = [o.seg["before_img"], o._image_features(img), o.seg["before_suffix"], optim, o.seg["after"], o.seg["target"]]
        else:
            parts = [o.seg["before"], optim, o.seg["after"], o.seg["target"]]
        loss = self._loss(self._rows(torch.cat(parts, dim=1)))[0]
        wanted = ([onehot] if cfg.gcg_attack else []) + ([img] if cfg.pgd_attack else [])
        grads = list(torch.autograd.grad(loss, wanted))
        return (grads.pop(0)[0].numpy() if cfg.gcg_attack else None), (grads.pop(0).numpy() if cfg.pgd_attack else None)


@functools.lru_cache(maxsize=None)
def _compared(kind, mode):
    """One traced run of the engine held to the recomputation, step by step; returns, per step with candidates, whether
    the winner comparison was skipped as a near-tie (top two recomputed losses within the tolerance)."""
    res, trace, cfg = run_mm(kind, mode)
    rc = _Recompute(kind, mode, cfg)
    assert len(trace) == cfg.num_steps == len(res.losses)
    image = rc.image0.numpy()
    ties = []
    for i, st in enumerate(trace):
        if i == 0:
            # the gradients of step 0 against torch autograd of the restated loss through the same model
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
    base, _, _ = run_mm("llava", "joint", trace=False)
    res, _, _ = run_mm("llava", "joint", trace=False, **engine)
    np.testing.assert_allclose(res.losses, base.losses, rtol=0, atol=1e-4)
    assert res.strings == base.strings
    base, _, _ = run_mm("llava", "gcg", trace=False)
    res, _, _ = run_mm("llava", "gcg", trace=False, **engine)
    np.testing.assert_allclose(res.losses, base.losses, rtol=0, atol=1e-4)
    assert res.strings == base.strings


def test_early_stop_is_still_the_argmax_test():
    """early_stop under the new rule: the run ends at the first step one of whose candidates has argmax(row) == label on
    every target row (recomputed here), not before and not later -- on a target for which that happens well before the
    last step (step 3 of 8 in the CPU reference run, test_mellowmax.py)."""
    E = R.EARLY
    res, trace, cfg = run_mm(E["kind"], E["mode"], steps=E["steps"], cfg_over=dict(early_stop=True), target=E["target"])
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


def test_default_rule_is_unchanged():
    """loss_rule left alone, and "ce" given explicitly: the golden trajectory of the default rule (g5_llava_gcg), as before."""
    import json
    from bimodalattack_amd import BimodalAttackConfig, run, synthetic as S
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    m = json.load(open(os.path.join(golden, "g5_meta.json")))["cases"]["llava_gcg"]
    z = np.load(os.path.join(golden, "g5_llava_gcg.npz"))
    out = []
    for rule in (None, "ce"):
        model, tok, proc, image = S.tiny_case(m["kind"], device=DEV)
        cfg = BimodalAttackConfig(seed=1, verbosity="ERROR", optim_str_init=m["optim_str_init"], use_mellowmax=True,
                                  images_folder=tempfile.mkdtemp(), **m["config"])
        out.append(run(model, tok, proc, m["goal"], m["goal"], m["target"], image, cfg, normalize=S.Normalize(S.CLIP_MEAN, S.CLIP_STD),
                       rng_device="cpu", strict=True, loss_rule=rule))
    assert out[0].losses == out[1].losses and out[0].strings == out[1].strings
    np.testing.assert_allclose(out[0].losses, z["losses"], rtol=1e-4)
    assert out[0].strings == m["strings"]


def test_bad_alpha_raises_when_the_rule_is_selected():
    with pytest.raises(ValueError, match="mellowmax_alpha"):
        run_mm("llava", "gcg", steps=1, cfg_over=dict(mellowmax_alpha=0.0), trace=False)
    run_mm("llava", "gcg", steps=1, cfg_over=dict(mellowmax_alpha=0.0), trace=False, loss_rule="ce")     # unread without it


def test_engine_keeps_the_rule_it_was_given():
    """The options object reaches the engine as from_env made it: the rule is an attribute, not a dataclass field, and must
    not be lost on the way."""
    from bimodalattack_amd import synthetic as S
    from bimodalattack_amd.attack import BimodalAttack
    from bimodalattack_amd.config import EngineOptions
    model, tok, proc, image = S.tiny_case("llava", device=DEV)
    atk = BimodalAttack(model, tok, proc, R.run_config("gcg", 1), None, EngineOptions.from_env(loss_rule="mellowmax", save_images=False))
    assert atk.opt.loss_rule == "mellowmax" and atk._mm_alpha == ALPHA
    atk = BimodalAttack(model, tok, proc, R.run_config("gcg", 1), None, EngineOptions.from_env(save_images=False))
    assert atk.opt.loss_rule == "ce" and atk._mm_alpha is None


@pytest.mark.parametrize("mode", ["gcg", "joint", "pgd"])
def test_no_host_reads_added(mode):
    from test_apgd_gpu import _HostReads
    counts = {}
    for rule in ("ce", "mellowmax"):
        run_mm("llava", mode, steps=2, trace=False, loss_rule=rule, filter_first=False)       # warm
        with _HostReads() as h:
            run_mm("llava", mode, steps=6, trace=False, loss_rule=rule, filter_first=False)
        counts[rule] = h.n
    assert counts["mellowmax"] == counts["ce"], counts
