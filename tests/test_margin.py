"""The Carlini-Wagner margin target loss (loss_rule="margin"; contract in include/bma.h, a2c) on the CPU: the float64
restatement against torch autograd and against the stated tie rule, three mutants of it told apart on the pools, the engine
options, the C entry point's argument checks, and the CPU reference runs that the engine tests (test_margin_gpu.py) are
held to.  The kernels meet the same restatement in test_margin_gpu.py."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import margin_ref as R

INF, NAN = float("inf"), float("nan")


def untied(B=4, T=5, V=37, seed=0):
    """(B, T, V) rows without a tie anywhere: a permutation of distinct eighths per row."""
    rs = np.random.RandomState(seed)
    return np.stack([[rs.permutation(V) / 8.0 - 2.0 for _ in range(T)] for _ in range(B)]).astype(np.float32)


@pytest.mark.parametrize("kappa", [0.0, 0.05, 1.5, INF])
def test_restatement_equals_torch_autograd_without_ties(kappa):
    z, lab = untied(), R.labels_for(5, 37)
    z[0, 1, 3] = NAN                                        # a NaN off the label: the row's margin is NaN, its gradient zero
    z[1, 2, lab[2]] = NAN                                   # a NaN at the label
    z[1, 3, lab[3]] = -INF                                  # a label of -inf beside finite logits: +inf, an active row
    z[2, 0, :] = -INF                                       # a row of -inf: NaN
    z[3, 1, lab[1]] = z[3, 1].max() + 4.0                   # the label is the row maximum: m < 0
    if np.isfinite(kappa) and kappa > 0:
        z[3, 2, lab[2]] = np.delete(z[3, 2], lab[2]).max() + np.float32(kappa)      # (float32 kappa below; m is near -kappa)
    ref = R.restated64(z, lab, kappa, grad_scale=3.0)
    loss, grad = R.autograd64(z, lab, kappa, grad_scale=3.0)
    assert np.isnan(ref["m"][0, 1]) and np.isnan(ref["m"][1, 2]) and ref["m"][1, 3] == INF and np.isnan(ref["m"][2, 0])
    assert np.array_equal(np.isnan(ref["loss"]), [True, True, True, False]) and ref["a"][1, 3] and not ref["a"][2, 0]
    assert np.array_equal(np.isnan(loss), np.isnan(ref["loss"]))
    np.testing.assert_allclose(ref["loss"][3], loss[3], rtol=0, atol=1e-14)
    # dlogits is d(grad_scale * loss)/dz with g = float32(3) / float32(5): torch's own backward of max, clamp and mean
    g32 = float(np.float32(3.0) / np.float32(5))
    assert set(np.unique(ref["dlogits"])) <= {0.0, g32, -g32}
    np.testing.assert_allclose(ref["dlogits"], np.nan_to_num(grad), rtol=0, atol=abs(g32 - 0.6) + 1e-15)
    assert np.array_equal(ref["dlogits"] != 0, np.nan_to_num(grad) != 0)
    assert (ref["dlogits"][0, 1] == 0).all() and (ref["dlogits"][2, 0] == 0).all()


def test_margin_exactly_minus_kappa_is_active():
    """torch.clamp's backward lets equality through; so does a_j.  kappa = 0.25 and eighths: m = -kappa exactly."""
    z, lab = untied(B=1, T=3, V=11), np.array([0, 4, 10])
    z[0, 1, 4] = np.delete(z[0, 1], 4).max() + 0.25
    ref = R.restated64(z, lab, 0.25)
    _, grad = R.autograd64(z, lab, 0.25)
    assert ref["m"][0, 1] == -0.25 and ref["a"][0, 1]
    assert grad[0, 1, 4] < 0 and np.array_equal(ref["dlogits"] != 0, grad != 0)
    assert not R.restated64(z, lab, 0.25, strict=True)["a"][0, 1]
    # kappa = +inf: nothing is clamped, every finite row is active
    z[0, 2, 10] = 100.0
    ref = R.restated64(z, lab, INF)
    assert ref["a"].all() and ref["loss"][0] == ref["m"][0].sum() / 3 and ref["m"][0, 2] < -90


def test_ties_resolve_to_the_first_index():
    z = np.full((1, 4, 9), -1.0, np.float32)
    lab = np.array([2, 0, 8, 4])
    z[0, 0, [1, 2, 5, 7]] = 3.0                             # label tied with the runner-ups: i = 1, m = 0, no hit (1 < 2)
    z[0, 1, [0, 3, 4]] = 2.0                                # label first among the tied: i = 3, m = 0, a hit
    z[0, 2, [6, 7]] = 5.0                                   # two runner-ups above the label: i = 6
    z[0, 3, :] = 0.5                                        # everything tied: i = 0 (4 is the label), no hit
    ref = R.restated64(z, lab, 0.0)
    assert ref["i"][0].tolist() == [1, 3, 6, 0] and ref["m"][0].tolist() == [0.0, 0.0, 6.0, 0.0]
    assert not ref["match"][0]
    assert R.restated64(z[:, 1:2], lab[1:2], 0.0)["match"][0] and not R.restated64(z[:, :1], lab[:1], 0.0)["match"][0]
    nz = np.argwhere(ref["dlogits"][0] != 0).tolist()
    assert nz == [[0, 1], [0, 2], [1, 0], [1, 3], [2, 6], [2, 8], [3, 0], [3, 4]]
    assert R.restated64(z, lab, 0.0, tie="last")["i"][0].tolist() == [7, 4, 7, 8]
    # every v != y NaN: no runner-up at all
    z[0, 0, :] = NAN
    z[0, 0, 2] = 1.0
    ref = R.restated64(z, lab, 0.0)
    assert ref["i"][0, 0] == -1 and np.isnan(ref["m"][0, 0]) and (ref["dlogits"][0, 0] == 0).all()
    # a label outside [0, V): the candidate is NaN and no match, that row is zeros, the others are written
    ref = R.restated64(z[:, 1:], np.array([0, 9, 4]), 0.0)
    assert np.isnan(ref["loss"][0]) and not ref["match"][0]
    assert (ref["dlogits"][0, 1] == 0).all() and (ref["dlogits"][0, 0] != 0).sum() == 2


def test_three_mutants_are_told_apart_on_the_pools():
    T, V, kappa = 5, 257, 2.0
    z, lab = R.grid_pool(8, T, V), R.labels_for(T, V)
    z[0, 1, lab[1]] = 20.0                                  # a label that is the row maximum ...
    z[1, 2, lab[2]] = np.delete(z[1, 2], lab[2]).max() + 2.0                 # ... and a margin of exactly -kappa
    ref = R.restated64(z, lab, kappa)
    assert ref["m"][0, 1] < 0 and ref["m"][1, 2] == -kappa
    ties = (z == z.max(-1, keepdims=True)).sum(-1)
    assert (ties > 1).mean() > 0.2, "the grid pool must be full of tied maxima"
    keep = R.restated64(z, lab, kappa, exclude_label=False)
    assert not np.array_equal(keep["m"], ref["m"]) and not np.array_equal(keep["loss"], ref["loss"])
    last = R.restated64(z, lab, kappa, tie="last")
    assert np.array_equal(last["m"], ref["m"]) and not np.array_equal(last["i"], ref["i"])
    assert not np.array_equal(last["dlogits"], ref["dlogits"])
    strict = R.restated64(z, lab, kappa, strict=True)
    assert np.array_equal(strict["loss"], ref["loss"]) and not np.array_equal(strict["dlogits"], ref["dlogits"])
    # the grid is exact: float32 margins and sums equal the float64 ones, so the expected loss is a cast
    m32 = ref["m"].astype(np.float32)
    assert np.array_equal(m32.astype(np.float64), ref["m"])
    acc = np.zeros(8, np.float32)
    for j in range(T):
        acc = acc + np.maximum(m32[:, j], np.float32(-kappa))
    assert np.array_equal(acc / np.float32(T), R.expected_loss32(ref))
    # the generic pool rounds: its float32 evaluation differs from float64 and stays inside the stated bound
    zg = R.generic_pool(8, T, V)
    rg = R.restated64(zg, lab, kappa)
    acc = np.zeros(8, np.float32)
    for j in range(T):
        o = np.delete(zg[:, j], lab[j], axis=-1).max(-1)
        acc = acc + np.maximum(o - zg[:, j, lab[j]], np.float32(-kappa))
    err = np.abs((acc / np.float32(T)).astype(np.float64) - rg["loss"])
    assert err.max() > 0 and (err <= R.loss_bound(rg, T, kappa)).all()


def test_margin_options(monkeypatch):
    import copy
    import dataclasses
    from bimodalattack_amd import BimodalAttackConfig
    from bimodalattack_amd.config import EngineOptions
    monkeypatch.delenv("BMA_LOSS_RULE", raising=False)
    monkeypatch.delenv("BMA_MARGIN_KAPPA", raising=False)
    o = EngineOptions.from_env()
    assert o.loss_rule == "ce" and o.margin_kappa == 0.0 and EngineOptions().margin_kappa == 0.0
    o = EngineOptions.from_env(loss_rule="margin", margin_kappa=0.05)
    assert o.loss_rule == "margin" and o.margin_kappa == 0.05
    assert EngineOptions.from_env().margin_kappa == 0.0                        # an instance's choice stays its own
    assert EngineOptions.from_env(margin_kappa=INF).margin_kappa == INF and EngineOptions.from_env(margin_kappa=2).margin_kappa == 2.0
    monkeypatch.setenv("BMA_LOSS_RULE", "margin")
    monkeypatch.setenv("BMA_MARGIN_KAPPA", "0.5")
    e = EngineOptions.from_env()
    assert e.loss_rule == "margin" and e.margin_kappa == 0.5
    assert EngineOptions.from_env(margin_kappa=0.25, loss_rule="ce") == EngineOptions.from_env(loss_rule="ce", margin_kappa=0.25)
    assert EngineOptions.from_env(margin_kappa=0.25).margin_kappa == 0.25      # the keyword wins over the environment
    monkeypatch.setenv("BMA_MARGIN_KAPPA", "inf")
    assert EngineOptions.from_env().margin_kappa == INF
    for bad in ("-1", "nan", "much", ""):
        monkeypatch.setenv("BMA_MARGIN_KAPPA", bad)
        with pytest.raises(ValueError, match="margin_kappa"):
            EngineOptions.from_env()
    monkeypatch.delenv("BMA_MARGIN_KAPPA")
    monkeypatch.delenv("BMA_LOSS_RULE")
    for bad in (True, NAN, -0.5, -INF, "0.1"):
        with pytest.raises(ValueError, match="margin_kappa"):
            EngineOptions.from_env(margin_kappa=bad)
    with pytest.raises(ValueError, match="loss_rule"):
        EngineOptions.from_env(loss_rule="Margin")
    # attributes beside the dataclass fields: repr, ==, copies
    assert copy.copy(o).margin_kappa == 0.05 and copy.deepcopy(o).loss_rule == "margin"
    assert "loss_rule='margin'" in repr(o) and "margin_kappa=0.05" in repr(o) and "margin_kappa=0.0" in repr(EngineOptions())
    assert o != EngineOptions.from_env(loss_rule="margin") and o == EngineOptions.from_env(loss_rule="margin", margin_kappa=0.05)
    assert len(dataclasses.fields(BimodalAttackConfig)) == 27
    assert "margin_kappa" not in {f.name for f in dataclasses.fields(EngineOptions)}


def test_entry_points_are_exported_and_validate_without_a_device():
    from bimodalattack_amd import native, ops
    from bimodalattack_amd.native import lib
    raw = ctypes.CDLL(native.LIB_PATH)
    for name in ("bma_margin_target_ws_bytes", "bma_margin_target"):
        assert hasattr(raw, name) and name in native.PROTOTYPES
    assert callable(ops.margin_target) and issubclass(ops.TargetMargin, torch.autograd.Function)
    assert native.KERNEL_IDS["margin"] == 23 and native.KERNEL_IDS["margin_dlogits"] == 24
    for slot in ("margin", "margin_dlogits"):
        assert lib.bma_profile_kernel_name(native.KERNEL_IDS[slot]) not in (None, b"?")
    assert lib.bma_profile_kernel_name(25) in (None, b"?")
    assert lib.bma_margin_target_ws_bytes(512, 20) == 3 * 512 * 20 * 4 and lib.bma_margin_target_ws_bytes(-1, 20) == 0
    x, lab, ws, loss, mt, dl = 64, 128, 192, 256, 320, 384
    f = lib.bma_margin_target
    assert f(x, 40, 10, lab, 0, 4, 10, 0, 0.0, ws, loss, None, None, 1.0, None) == 0          # B == 0: nothing to do
    assert f(None, 40, 10, lab, 4, 4, 10, 0, 0.0, ws, loss, None, None, 1.0, None) == -1      # null pointers
    assert f(x, 40, 10, None, 4, 4, 10, 0, 0.0, ws, loss, None, None, 1.0, None) == -1
    assert f(x, 40, 10, lab, 4, 4, 10, 0, 0.0, None, loss, None, None, 1.0, None) == -1
    assert f(x, 40, 10, lab, 4, 4, 10, 0, 0.0, ws, None, None, None, 1.0, None) == -1
    assert f(x, 40, 10, lab, 4, 0, 10, 0, 0.0, ws, loss, None, None, 1.0, None) == -1         # T < 1
    assert f(x, 40, 10, lab, -1, 4, 10, 0, 0.0, ws, loss, None, None, 1.0, None) == -1        # B < 0
    assert f(x, 40, 9, lab, 4, 4, 10, 0, 0.0, ws, loss, None, None, 1.0, None) == -1          # rows shorter than V
    assert f(x, 4, 1, lab, 4, 4, 1, 0, 0.0, ws, loss, None, None, 1.0, None) == -1            # V < 2: no wrong logit
    for kappa in (-1.0, -0.0001, -INF, NAN):
        assert f(x, 40, 10, lab, 4, 4, 10, 0, kappa, ws, loss, None, None, 1.0, None) == -1
    assert f(x, 40, 10, lab, 4, 4, 10, 7, 0.0, ws, loss, None, None, 1.0, None) == -2         # dtype
    assert f(x, 40, 10, lab, 4, 4, 10, 0, 0.0, ws + 2, loss, None, None, 1.0, None) == -3     # misaligned
    assert f(x, 40, 10, lab, 4, 4, 10, 0, INF, ws, loss, mt + 2, None, 1.0, None) == -3       # (kappa = +inf is allowed)
    assert f(x, 40, 10, lab, 4, 4, 10, 1, 0.0, ws, loss, None, dl + 1, 1.0, None) == -3       # dlogits off the element grid


def test_wrappers_refuse_cpu_tensors():
    from bimodalattack_amd import ops
    x, lab = torch.zeros(1, 2, 8), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        ops.margin_target(x, lab, 0.0)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        ops.TargetMargin.apply(x[0], lab, 0.0)


@functools.lru_cache(maxsize=None)
def _reference_runs():
    return {case: R.reference_run(*case) for case in R.CASES}


def test_reference_runs_stay_clear_of_ties():
    """Conditions on the CPU reference alone, at the seeds of the engine tests: at most 5 % of the scoring steps have their
    two best candidate losses within the engine tests' tolerance, and no gradient site is fragile (two best non-label
    logits of a row, or a margin and -kappa, within it)."""
    ties, fragile = [], []
    for case, (res, trace, notes, grad_notes) in _reference_runs().items():
        assert len(res["losses"]) == 4 and np.isfinite(res["losses"]).all()
        ties += [n["near_tie"] for n in notes]
        fragile += [n["fragile"] for n in grad_notes]
    assert len(ties) == 16 and np.mean(ties) <= 0.05, ties
    assert len(fragile) == 24 and not any(fragile), fragile


def test_reference_runs_reach_the_clamp():
    """kappa = 0.05 is not idle in the runs: some step's winner has a row already below -kappa."""
    runs = _reference_runs()
    assert any(n["clamped"] for (_, _, notes, _) in runs.values() for n in notes)
    # (llava/joint and gemma3/gcg: one of T = 5 rows at step 3, so the loss sits kappa/T = 0.01 below its kappa = 0 value)
    for case in (("llava", "joint"), ("gemma3", "gcg")):
        assert runs[case][2][3]["clamped"]
        free = R.reference_run(*case, kappa=0.0)[0]["losses"]
        assert abs((free[3] - runs[case][0]["losses"][3]) - R.RUN_KAPPA / 5) <= 1e-6
        assert free[:3] == runs[case][0]["losses"][:3]


def test_reference_early_stop_run():
    E = R.EARLY
    res, trace, notes, _ = R.reference_run(E["kind"], E["mode"], E["steps"], E["target"], early_stop=True)
    assert [n["hit"] for n in notes] == [False, False, True] and len(res["losses"]) == 3
    assert res["losses"][-1] == float(np.float32(-R.RUN_KAPPA))          # T = 1: the won row, clamped
