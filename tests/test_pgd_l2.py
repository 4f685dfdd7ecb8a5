"""The L2-ball threat model of the PGD image update (``pgd_norm="l2"``; the reference has no L2 update) on the CPU: the
``pgd_norm`` engine option, the torch restatement (oracle/kernels.py) of the arithmetic contract of include/bma.h (section a5c) with the properties
a projection onto the ball must have, and the C entry points' argument checks.  The kernels are held to the same
restatement, bit for bit, in test_pgd_l2_gpu.py.  The restatement never calls the library."""

import math

import numpy as np
import pytest
import torch

from oracle.kernels import ULP, apgd_l2_restated, dist64, l2_restated
from oracle.kernels import as_f32 as _t, f32_scalar as _s, l2_clamp01 as _clamp01, l2_descent as _descent


# ------------------------------------------------------------------ the option
def test_pgd_norm_option(monkeypatch):
    import dataclasses
    from bimodalattack_amd import BimodalAttackConfig
    from bimodalattack_amd.config import EngineOptions
    monkeypatch.delenv("BMA_PGD_NORM", raising=False)
    monkeypatch.delenv("BMA_PGD_RULE", raising=False)
    assert EngineOptions.from_env().pgd_norm == "linf"
    assert EngineOptions.from_env(pgd_norm="l2").pgd_norm == "l2"
    monkeypatch.setenv("BMA_PGD_NORM", "l2")
    assert EngineOptions.from_env().pgd_norm == "l2"
    assert EngineOptions.from_env(pgd_norm="linf").pgd_norm == "linf"          # the keyword wins over the environment
    # orthogonal to the rule
    o = EngineOptions.from_env(pgd_rule="apgd")
    assert (o.pgd_rule, o.pgd_norm) == ("apgd", "l2")
    monkeypatch.setenv("BMA_PGD_NORM", "l1")
    with pytest.raises(ValueError, match="pgd_norm"):
        EngineOptions.from_env()
    monkeypatch.delenv("BMA_PGD_NORM")
    with pytest.raises(ValueError, match="pgd_norm"):
        EngineOptions.from_env(pgd_norm="L2")
    # "l2" is a norm, not a rule
    monkeypatch.setenv("BMA_PGD_RULE", "l2")
    with pytest.raises(ValueError, match="pgd_rule"):
        EngineOptions.from_env()
    monkeypatch.delenv("BMA_PGD_RULE")
    # an engine option, not a config field: the dataclass stays the reference's 27 fields
    assert len(dataclasses.fields(BimodalAttackConfig)) == 27
    assert "pgd_norm" not in {f.name for f in dataclasses.fields(BimodalAttackConfig)}


def test_apgd_state_takes_the_norm():
    from bimodalattack_amd.pgd import ApgdState
    a, b = ApgdState(0.5), ApgdState(0.5, "l2")
    assert (a.norm, b.norm) == ("linf", "l2")
    # the host logic does not depend on the norm: eta starts at 2*eps, alpha plays no part
    seq = [None, 3.0, 2.5, 2.6, 2.4, 2.4, 2.3, 2.2, 2.25, 2.1, 2.0, 2.0]
    assert [a.decide(l, i) for i, l in enumerate(seq)] == [b.decide(l, i) for i, l in enumerate(seq)]
    assert b.last is not None and ApgdState(0.25, "l2").decide(None, 0) == (0.5, False, False)
    with pytest.raises(ValueError, match="norm"):
        ApgdState(0.5, "l1")


# ------------------------------------------------------------------ the restatement
N = 3 * 64 * 64                         # diameter of the [0,1] cube: sqrt(N) = 110.9
# The radii.  The contract's bound below is RELATIVE (one fp32 rounding each of f and of the product d*f, on top of the one of
# the norm), but the sum x0 + d*f also rounds, at the pixel's own ulp (<= 2^-25 absolute) whatever eps is: summed over random
# signs that moves the distance by about 2^-24 / sqrt(12) = 1.7e-8 absolute.  The relative slack the bound leaves beyond the
# roundings of the norm and f (2 * 2^-24 * eps) covers five of those from eps = 0.5 up, which is also where the L2 budgets
# of the literature start (0.5 on CIFAR-sized, 3 on ImageNet-sized images).  200 lies beyond the cube's diameter.
RADII = (0.5, 2.0, 16.0, 64.0, 200.0)


def _inputs(seed, n=N):
    rs = np.random.RandomState(seed)
    x0 = rs.uniform(0, 1, n).astype(np.float32)
    x = np.clip(x0 + rs.uniform(-0.3, 0.3, n), 0, 1).astype(np.float32)
    prev = np.clip(x0 + rs.uniform(-0.3, 0.3, n), 0, 1).astype(np.float32)
    best = rs.uniform(0, 1, n).astype(np.float32)
    g = rs.standard_normal(n).astype(np.float32)
    return x, g, x0, prev, best


@pytest.mark.parametrize("eps", RADII)
def test_restated_step_lands_in_the_ball_and_the_cube(eps):
    x, g, x0, prev, best = _inputs(int(eps * 10))
    bound = eps * (1 + 4 * ULP)
    for step in (0.25 * eps, 2 * eps, 40.0):
        out, norms = l2_restated(x, g, x0, eps, step)
        d = dist64(out, x0)
        print(f"l2   eps {eps} step {step}: |out-x0| = {d!r}  bound {bound!r}  norms {norms.tolist()}")
        assert out.min() >= 0 and out.max() <= 1
        assert d <= bound
        new, p, b, norms = apgd_l2_restated(x, g, x0, prev, best, eps, step, True, False)
        d = dist64(new, x0)
        print(f"apgd eps {eps} eta  {step}: |new-x0| = {d!r}  bound {bound!r}  norms {norms.tolist()}")
        assert new.min() >= 0 and new.max() <= 1
        assert d <= bound
        assert np.array_equal(p, x) and np.array_equal(b, new)
    # a step of length 40 leaves the small balls (the projection is active) and cannot leave the one beyond the diameter
    _, norms = l2_restated(x, g, x0, eps, 40.0)
    if eps <= 16.0:
        assert norms[1] > eps
    if eps == 200.0:
        assert norms[1] < eps


def _sterbenz_inputs(seed, n=N):
    """Pixels for which P is the identity BIT FOR BIT when the ball is idle: x0 + (y - x0) returns y exactly only when
    y - x0 is exact, which Sterbenz's lemma gives for x0/2 <= y <= 2*x0.  x0 in [0.3, 0.7] and |y - x0| <= 0.15 keep every
    pixel there (and inside (0, 1), so clamp01 is idle too)."""
    rs = np.random.RandomState(seed)
    x0 = rs.uniform(0.3, 0.7, n).astype(np.float32)
    x = (x0 + rs.uniform(-0.1, 0.1, n)).astype(np.float32)
    g = rs.standard_normal(n).astype(np.float32)
    return x, g, x0


def test_restated_step_with_an_idle_ball_is_the_clamped_descent_step():
    eps, step = 200.0, 0.04              # |step * u| <= 0.04: y stays within 0.15 of x0
    x, g, x0 = _sterbenz_inputs(7)
    out, norms = l2_restated(x, g, x0, eps, step)
    y, _ = _descent(_t(x), _t(g), _s(step))
    assert float(norms[1]) < eps
    assert np.array_equal(out.view(np.uint32), _clamp01(y).numpy().view(np.uint32))
    # any pixels (clamp active, y far from x0): the same up to the roundings of y - x0 and of the sum, 2^-25 each
    x, g, x0, _, _ = _inputs(8)
    out, _ = l2_restated(x, g, x0, eps, 0.5)
    y, _ = _descent(_t(x), _t(g), _s(0.5))
    assert np.abs(out.astype(np.float64) - _clamp01(y).numpy().astype(np.float64)).max() <= ULP


def test_restated_step_with_a_zero_gradient_keeps_a_feasible_image():
    x, _, x0 = _sterbenz_inputs(9)
    g = np.zeros_like(x)
    d = dist64(x, x0)
    for eps in (math.ceil(d), 200.0):    # feasible: inside the ball and the cube
        out, norms = l2_restated(x, g, x0, eps, 0.25 * eps)
        assert norms[0] == 0 and float(norms[1]) <= eps
        assert np.array_equal(out.view(np.uint32), x.view(np.uint32))
    # auto-PGD with prev == x: z = x, m = x, new = x
    new, p, b, _ = apgd_l2_restated(x, g, x0, x.copy(), x.copy(), 200.0, 400.0, False, False)
    assert np.array_equal(new.view(np.uint32), x.view(np.uint32)) and np.array_equal(p, x) and np.array_equal(b, x)


def test_restated_corners():
    x, g, x0, prev, best = _inputs(11, 4099)
    # x == x0, g == 0: the norm of y - x0 is zero, eps / 0 = inf, f = 1 (not NaN)
    out, norms = l2_restated(x0, np.zeros_like(x0), x0, 0.5, 0.1)
    assert norms.tolist() == [0.0, 0.0] and np.array_equal(out, x0)
    # one NaN in g reaches every pixel through the norm
    g2 = g.copy()
    g2[17] = np.nan
    out, norms = l2_restated(x, g2, x0, 0.5, 0.1)
    assert np.isnan(out).all() and np.isnan(norms).all()
    new, p, b, norms = apgd_l2_restated(x, g2, x0, prev, best, 0.5, 1.0, True, True)
    assert np.isnan(new).all() and np.isnan(p).all() and np.isnan(b).all() and np.isnan(norms).all()
    # the flags: prev / best as bma_apgd_step
    for take_best in (False, True):
        for restart in (False, True):
            new, p, b, norms = apgd_l2_restated(x, g, x0, prev, best, 2.0, 4.0, take_best, restart)
            if restart and not take_best:
                assert norms is None and all(np.array_equal(a, best) for a in (new, p, b))
                continue
            assert np.array_equal(b, new if take_best else best)
            assert np.array_equal(p, new if restart else x)


# ------------------------------------------------------------------ the C entry points
def test_l2_entry_points_are_exported_and_validate_without_a_device():
    import ctypes
    from bimodalattack_amd import native
    from bimodalattack_amd.native import lib
    raw = ctypes.CDLL(native.LIB_PATH)
    for name in ("bma_l2_ws_bytes", "bma_l2_step", "bma_apgd_l2_step"):
        assert hasattr(raw, name) and name in native.PROTOTYPES
    assert lib.bma_version() == 114 and native.ABI_VERSION == 114
    assert native.KERNEL_IDS["l2"] == 20 and native.lib.bma_profile_kernel_name(20) not in (None, b"?")
    assert lib.bma_l2_ws_bytes(0) == 0
    ws_bytes = lib.bma_l2_ws_bytes(3 * 896 * 896)
    assert 0 < ws_bytes <= 3 * 2048 * 8 and ws_bytes % 8 == 0                  # <= 2048 fp64 partials per norm
    assert lib.bma_l2_ws_bytes(5) == ws_bytes                                   # the caller allocates once, for any image
    a, b, c, d, e, o, ws, nm = 16, 32, 48, 64, 80, 96, 112, 128
    # plain
    assert lib.bma_l2_step(None, None, None, -1, 0.5, 0.1, None, None, None, None) == -1
    assert lib.bma_l2_step(None, None, None, 0, 0.5, 0.1, None, None, None, None) == 0
    assert lib.bma_l2_step(a, b, c, 8, 0.5, 0.1, o, None, nm, None) == -1                 # no workspace
    assert lib.bma_l2_step(a, b, c, 8, 0.5, 0.1, o, ws, None, None) == -1                 # no norms
    assert lib.bma_l2_step(a, b, None, 8, 0.5, 0.1, o, ws, nm, None) == -1
    assert lib.bma_l2_step(a + 2, b, c, 8, 0.5, 0.1, o, ws, nm, None) == -3               # misaligned
    assert lib.bma_l2_step(a, b, c, 8, 0.5, 0.1, o, ws + 4, nm, None) == -3               # fp64 partials
    assert lib.bma_l2_step(a, b, c, 8, 0.5, 0.1, o, ws, nm + 1, None) == -3
    # auto-PGD
    assert lib.bma_apgd_l2_step(None, None, None, None, None, -1, 0.5, 1.0, 0, 0, None, None, None, None) == -1
    assert lib.bma_apgd_l2_step(None, None, None, None, None, 0, 0.5, 1.0, 0, 0, None, None, None, None) == 0
    assert lib.bma_apgd_l2_step(a, b, c, d, e, 8, 0.5, 1.0, 0, 0, o, None, nm, None) == -1
    assert lib.bma_apgd_l2_step(a, b, c, d, e, 8, 0.5, 1.0, 0, 0, o, ws, None, None) == -1
    assert lib.bma_apgd_l2_step(a, b, c, None, e, 8, 0.5, 1.0, 0, 0, o, ws, nm, None) == -1
    assert lib.bma_apgd_l2_step(a, b, c, d, e, 8, 0.5, 1.0, 2, 0, o, ws, nm, None) == -1   # a flag is 0 or 1
    assert lib.bma_apgd_l2_step(a, b, c, d, e, 8, 0.5, 1.0, 0, -1, o, ws, nm, None) == -1
    assert lib.bma_apgd_l2_step(a, b, c, d, d, 8, 0.5, 1.0, 0, 0, o, ws, nm, None) == -1   # prev == best
    assert lib.bma_apgd_l2_step(a, b, c, a, e, 8, 0.5, 1.0, 0, 0, o, ws, nm, None) == -1   # prev == x
    assert lib.bma_apgd_l2_step(a, b, c, d, o, 8, 0.5, 1.0, 0, 0, o, ws, nm, None) == -1   # best == out
    assert lib.bma_apgd_l2_step(a + 2, b, c, d, e, 8, 0.5, 1.0, 0, 0, o, ws, nm, None) == -3
    assert lib.bma_apgd_l2_step(a, b, c, d, e + 1, 8, 0.5, 1.0, 1, 1, o, ws, nm, None) == -3


def test_l2_wrappers_refuse_cpu_tensors():
    from bimodalattack_amd import ops
    x = torch.zeros(8)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        ops.l2_step(x, x, x, 0.5, 0.1)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        ops.apgd_l2_step(x, x, x, x.clone(), x.clone(), 0.5, 1.0, False, False)
