"""The mellowmax target loss (loss_rule="mellowmax"; reference bimodalattack/utils.py:35-36 applied to the negated raw
target logits, as nanoGCG applies it) on the CPU: the float64 restatement against the reference's own outputs
(tests/golden/g9_mellowmax_unit.npz), the float32 restatement of the kernel's operation order against the float64 one, the
engine option, and the C entry point's argument checks.  The kernels are held to the same references in
test_mellowmax_gpu.py."""

import ctypes
import os

import numpy as np
import pytest
import torch

import mellowmax_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden():
    z = np.load(os.path.join(GOLDEN, "g9_mellowmax_unit.npz"))
    assert tuple(z["alphas"]) == R.ALPHAS and tuple(z["Ts"]) == (1, 2, 20, 65)
    return z


def golden_cases():
    """(T, alpha, logits, labels, out32, out64) of every recorded call."""
    z = golden()
    return [(int(T), float(a), z[f"T{T}_logits"], z[f"T{T}_labels"], z[f"T{T}_a{a}_out32"], z[f"T{T}_a{a}_out64"])
            for T in z["Ts"] for a in z["alphas"]]


def test_golden_covers_what_it_promises():
    for T, alpha, logits, labels, o32, o64 in golden_cases():
        t = R.gather_t(logits, labels)
        assert labels[-1] == logits.shape[2] - 1 and (T == 1 or labels[0] == 0)
        assert (alpha * t[12:16].max(-1) > 88).all() and np.isfinite(o64[:16]).all()
        assert np.isnan(o64[16]) and o64[17] == np.inf and o64[18] == -np.inf
        assert np.isnan(logits[0]).any() and np.isfinite(o64[0])             # a NaN off the label columns is never read
        for dt in (torch.bfloat16, torch.float16):
            x = torch.from_numpy(logits)
            assert torch.equal(x.to(dt).float().nan_to_num(7.0), x.nan_to_num(7.0))


def test_float64_restatement_equals_the_reference():
    for T, alpha, logits, labels, o32, o64 in golden_cases():
        t = R.gather_t(logits, labels)
        loss, w = R.restated64(t, alpha)
        assert R.same_special(loss, o64), (T, alpha)
        ok = np.isfinite(o64)
        # fp64 rounding: log / exp / the T-term sum, at the magnitude of alpha*t (<= 128) over alpha
        np.testing.assert_allclose(loss[ok], o64[ok], rtol=0, atol=64 * np.finfo(np.float64).eps * 128 / alpha)
        # the torch restatement of the function IS the reference's function (up to the order in which a CPU build of
        # torch happens to add the T terms)
        l32 = R.torch_mellowmax(torch.from_numpy(np.ascontiguousarray(t)), alpha).numpy()
        assert R.same_special(l32, o32) and R.same_special(R.autograd64(t, alpha)[0], o64)
        np.testing.assert_allclose(l32[ok], o32[ok], rtol=4 * np.finfo(np.float32).eps, atol=0)
        np.testing.assert_allclose(R.autograd64(t, alpha)[0][ok], o64[ok], rtol=0, atol=64 * np.finfo(np.float64).eps * 128 / alpha)
        # the weights: torch's own backward of the function, NaN patterns of the special rows included
        g = R.autograd64(t, alpha)[1]
        assert np.array_equal(np.isnan(w), np.isnan(g)), (T, alpha)
        np.testing.assert_allclose(w[~np.isnan(g)], g[~np.isnan(g)], rtol=0, atol=1e-13)
        if T == 1:
            assert np.array_equal(loss[:16], t[:16, 0].astype(np.float64))       # T = 1: the loss is t_0


def test_float32_kernel_order_against_float64():
    """The kernel's order of operations in float32 stays inside the bound the kernel itself is held to: 4 x the fp32 torch
    evaluation's own error per (T, alpha) class."""
    for T, alpha, logits, labels, o32, o64 in golden_cases():
        t = R.gather_t(logits, labels)
        loss, w = R.restated32_kernel_order(t, alpha)
        assert R.same_special(loss, o64), (T, alpha)
        ok = np.isfinite(o64)
        bound = 4.0 * np.abs(o32[ok].astype(np.float64) - o64[ok]).max()
        assert np.abs(loss[ok].astype(np.float64) - o64[ok]).max() <= bound, (T, alpha, bound)
    for T in (63, 64, 65, 257, 1025):                       # one wave, its edge, a workgroup's first sweep and beyond
        t = R.pool(T)
        for alpha in R.ALPHAS:
            lb, wb = R.bounds(t, alpha)
            l64, w64 = R.restated64(t, alpha)
            loss, w = R.restated32_kernel_order(t, alpha)
            assert np.abs(loss - l64).max() <= lb and np.abs(w - w64).max() <= wb, (T, alpha, lb, wb)


def test_loss_rule_option(monkeypatch):
    import dataclasses
    from bimodalattack_amd import BimodalAttackConfig, GCGConfig
    from bimodalattack_amd.config import EngineOptions, mellowmax_alpha
    monkeypatch.delenv("BMA_LOSS_RULE", raising=False)
    assert EngineOptions.from_env().loss_rule == "ce" and EngineOptions().loss_rule == "ce"
    assert EngineOptions.from_env(loss_rule="mellowmax").loss_rule == "mellowmax"
    assert EngineOptions.from_env().loss_rule == "ce"                          # an instance's choice stays its own
    monkeypatch.setenv("BMA_LOSS_RULE", "mellowmax")
    assert EngineOptions.from_env().loss_rule == "mellowmax"
    assert EngineOptions.from_env(loss_rule="ce").loss_rule == "ce"            # the keyword wins over the environment
    monkeypatch.setenv("BMA_LOSS_RULE", "mellow")
    with pytest.raises(ValueError, match="loss_rule"):
        EngineOptions.from_env()
    monkeypatch.delenv("BMA_LOSS_RULE")
    with pytest.raises(ValueError, match="loss_rule"):
        EngineOptions.from_env(loss_rule="Mellowmax")
    # use_mellowmax alone selects nothing: the dataclass behaves as the reference's, which never reads the field
    assert GCGConfig is BimodalAttackConfig
    cfg = GCGConfig(use_mellowmax=True, mellowmax_alpha=0.0)
    assert EngineOptions.from_env().loss_rule == "ce"
    assert len(dataclasses.fields(BimodalAttackConfig)) == 27
    assert "loss_rule" not in {f.name for f in dataclasses.fields(BimodalAttackConfig)}
    # alpha is read -- and checked -- under the rule only
    assert mellowmax_alpha(GCGConfig(mellowmax_alpha=0.5)) == 0.5 and mellowmax_alpha(GCGConfig()) == 1.0
    for bad in (0.0, -1.0, float("inf"), float("nan"), None, "1", True):
        with pytest.raises(ValueError, match="mellowmax_alpha"):
            mellowmax_alpha(GCGConfig(mellowmax_alpha=bad))
    assert cfg.mellowmax_alpha == 0.0                                          # untouched without the rule


def test_options_keep_the_rule_when_copied():
    """loss_rule is an attribute beside the dataclass fields: it shows in repr, and plain copies keep it."""
    import copy
    from bimodalattack_amd.config import EngineOptions
    o = EngineOptions.from_env(loss_rule="mellowmax")
    assert copy.copy(o).loss_rule == "mellowmax" and copy.deepcopy(o).loss_rule == "mellowmax"
    assert "loss_rule='mellowmax'" in repr(o) and "loss_rule='ce'" in repr(EngineOptions())
    assert o != EngineOptions.from_env() and o == EngineOptions.from_env(loss_rule="mellowmax")


def test_reference_runs_stay_clear_of_near_ties():
    """The seeds of the engine tests (test_mellowmax_gpu.py), on the CPU reference alone: at most 5 % of the steps with
    candidates have their two best losses within the engine tests' tolerance; and the early-stop run does stop early."""
    ties = []
    for kind, mode in R.CASES:
        res, trace, notes = R.reference_run(kind, mode)
        assert len(res["losses"]) == 4 and np.isfinite(res["losses"]).all()
        ties += [n["near_tie"] for n in notes]
    assert len(ties) == 16 and np.mean(ties) <= 0.05, ties
    E = R.EARLY
    res, trace, notes = R.reference_run(E["kind"], E["mode"], E["steps"], E["target"], early_stop=True)
    hits = [n["hit"] for n in notes]
    assert hits.index(True) == len(hits) - 1 == len(res["losses"]) - 1 < E["steps"] - 2, hits


def test_entry_point_is_exported_and_validates_without_a_device():
    from bimodalattack_amd import native
    from bimodalattack_amd.native import lib
    raw = ctypes.CDLL(native.LIB_PATH)
    for name in ("bma_mellowmax_target_ws_bytes", "bma_mellowmax_target"):
        assert hasattr(raw, name) and name in native.PROTOTYPES
    for slot in ("mellowmax", "mellowmax_dlogits"):
        assert native.lib.bma_profile_kernel_name(native.KERNEL_IDS[slot]) not in (None, b"?")
    assert lib.bma_mellowmax_target_ws_bytes(512, 20) == 512 * 20 * 4 and lib.bma_mellowmax_target_ws_bytes(-1, 20) == 0
    x, lab, ws, loss, dl = 64, 128, 192, 256, 320
    f = lib.bma_mellowmax_target
    assert f(x, 40, 10, lab, 0, 4, 10, 0, 1.0, ws, loss, None, 1.0, None) == 0          # B == 0: nothing to do
    assert f(None, 40, 10, lab, 4, 4, 10, 0, 1.0, ws, loss, None, 1.0, None) == -1      # null pointers
    assert f(x, 40, 10, None, 4, 4, 10, 0, 1.0, ws, loss, None, 1.0, None) == -1
    assert f(x, 40, 10, lab, 4, 4, 10, 0, 1.0, None, loss, None, 1.0, None) == -1
    assert f(x, 40, 10, lab, 4, 4, 10, 0, 1.0, ws, None, None, 1.0, None) == -1
    assert f(x, 40, 10, lab, 4, 0, 10, 0, 1.0, ws, loss, None, 1.0, None) == -1         # T < 1
    assert f(x, 40, 10, lab, -1, 4, 10, 0, 1.0, ws, loss, None, 1.0, None) == -1        # B < 0
    assert f(x, 40, 9, lab, 4, 4, 10, 0, 1.0, ws, loss, None, 1.0, None) == -1          # rows shorter than V
    for alpha in (0.0, -1.0, float("inf"), float("nan")):
        assert f(x, 40, 10, lab, 4, 4, 10, 0, alpha, ws, loss, None, 1.0, None) == -1
    assert f(x, 40, 10, lab, 4, 4, 10, 7, 1.0, ws, loss, None, 1.0, None) == -2         # dtype
    assert f(x, 40, 10, lab, 4, 4, 10, 0, 1.0, ws + 2, loss, None, 1.0, None) == -3     # misaligned
    assert f(x, 40, 10, lab, 4, 4, 10, 1, 1.0, ws, loss, dl + 1, 1.0, None) == -3       # dlogits off the element grid


def test_wrappers_refuse_cpu_tensors_and_bad_alpha():
    from bimodalattack_amd import ops
    x, lab = torch.zeros(1, 2, 8), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        ops.mellowmax_target(x, lab, 1.0)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        ops.TargetMellowmax.apply(x[0], lab, 1.0)
