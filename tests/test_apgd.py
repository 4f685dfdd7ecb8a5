"""The auto-PGD image update (reference bimodal_attack.py:1039-1110, ``perform_autopgd_step``) on the CPU: the float32
restatement of the rule (oracle/kernels.py) equal bit for bit to the reference's own outputs (tests/golden/g8_apgd_unit.npz), the host-state
class's eta / flag sequence, the C entry point's argument checks, and the ``pgd_rule`` engine option.  The kernel itself
is held to the same restatement in test_apgd_gpu.py."""

import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
from oracle.kernels import apgd_restated, same_bits


def unit_calls():
    """(i, current_loss, x, g, record) of every call in g8_apgd_unit."""
    z = np.load(os.path.join(GOLDEN, "g8_apgd_unit.npz"))
    out = []
    for i in range(int(z["n_calls"])):
        cur = float(z["losses"][i]) if bool(z["has_loss"][i]) else None
        out.append((i, cur, z[f"c{i}_x"], z[f"c{i}_g"], {k: z[f"c{i}_{k}"] for k in (
            "out", "prev", "best", "eta", "eta_used", "take_best", "restart", "count", "best_loss")}))
    return z, out


def test_restatement_equals_the_reference_bit_for_bit():
    z, calls = unit_calls()
    x0, eps = z["x0"], float(z["eps"])
    prev = best = None
    seen = set()
    for i, cur, x, g, rec in calls:
        if prev is None:
            prev, best = x.copy(), x.copy()
        tb, rst = bool(rec["take_best"]), bool(rec["restart"])
        out, prev, best = apgd_restated(x, g, x0, prev, best, eps, float(rec["eta_used"]), tb, rst)
        assert same_bits(out, rec["out"]), f"call {i}: output"
        assert same_bits(prev, rec["prev"]), f"call {i}: prev"
        assert same_bits(best, rec["best"]), f"call {i}: best"
        seen.add((tb, rst))
        # the fixtures reach the corners the comments promise
        assert np.isnan(out).any()
    assert {(True, False), (False, False), (False, True), (True, True)} <= seen
    assert np.signbit(z["c0_x"].reshape(-1)[1]) and z["c0_x"].reshape(-1)[1] == 0


def test_host_state_gives_the_reference_eta_and_flags():
    from bimodalattack_amd.pgd import ApgdState
    z, calls = unit_calls()
    st = ApgdState(float(z["eps"]))
    for i, cur, _, _, rec in calls:
        eta, take_best, restart = st.decide(cur, i)
        assert eta == float(rec["eta_used"]) and take_best == bool(rec["take_best"]) and restart == bool(rec["restart"]), i
        assert st.eta == float(rec["eta"]) and st.count == int(rec["count"]) and st.best_loss == float(rec["best_loss"]), i
    # a second run starts from scratch: eta = 2 * eps, config.alpha plays no part
    assert ApgdState(0.25).decide(None, 0) == (0.5, False, False)


def test_host_state_on_the_trajectory_goldens():
    """The reference's own losses of each g8 run fed to ApgdState reproduce its eta / restart sequence."""
    import json
    from bimodalattack_amd.pgd import ApgdState
    meta = json.load(open(os.path.join(GOLDEN, "g8_meta.json")))["cases"]
    assert set(meta) == {"llava_pgd", "llava_pgd_gcg", "llava_joint", "gemma3_pgd", "gemma3_joint"}
    for name, m in meta.items():
        z = np.load(os.path.join(GOLDEN, f"g8_{name}.npz"))
        st = ApgdState(m["config"]["eps"])
        restarts = []
        for i in range(m["steps"]):
            cur = float(z["losses"][i - 1]) if i else None
            eta, _, restart = st.decide(cur, i)
            assert eta == float(z[f"s{i}_eta_used"]) and restart == bool(z[f"s{i}_restart"]), (name, i)
            assert st.count == int(z[f"s{i}_count"]) and st.best_loss == float(z[f"s{i}_best_loss"]), (name, i)
            if restart:
                restarts.append(i)
        assert restarts == m["restarts"] and restarts, name


def test_apgd_entry_point_validation_launches_nothing():
    from bimodalattack_amd.native import lib
    a, b, c, d, e, o = 16, 32, 48, 64, 80, 96
    assert lib.bma_apgd_step(None, None, None, None, None, -1, 0.1, 0.2, 0, 0, None, None) == -1
    assert lib.bma_apgd_step(None, None, None, None, None, 0, 0.1, 0.2, 0, 0, None, None) == 0
    assert lib.bma_apgd_step(a, b, c, None, e, 8, 0.1, 0.2, 0, 0, o, None) == -1        # no prev
    assert lib.bma_apgd_step(a, b, c, d, e, 8, 0.1, 0.2, 2, 0, o, None) == -1           # a flag is 0 or 1
    assert lib.bma_apgd_step(a, b, c, d, e, 8, 0.1, 0.2, 0, -1, o, None) == -1
    assert lib.bma_apgd_step(a, b, c, d, d, 8, 0.1, 0.2, 0, 0, o, None) == -1           # prev == best
    assert lib.bma_apgd_step(a, b, c, a, e, 8, 0.1, 0.2, 0, 0, o, None) == -1           # prev == x
    assert lib.bma_apgd_step(a, b, c, d, o, 8, 0.1, 0.2, 0, 0, o, None) == -1           # best == out
    assert lib.bma_apgd_step(a + 2, b, c, d, e, 8, 0.1, 0.2, 0, 0, o, None) == -3       # misaligned
    assert lib.bma_apgd_step(a, b, c, d, e + 1, 8, 0.1, 0.2, 1, 1, o, None) == -3


def test_apgd_wrapper_refuses_cpu_tensors_and_aliased_state():
    import torch
    from bimodalattack_amd import ops
    x = torch.zeros(8)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        ops.apgd_step(x, x, x, x.clone(), x.clone(), 0.1, 0.2, False, False)


def test_pgd_rule_option(monkeypatch):
    import dataclasses
    from bimodalattack_amd import BimodalAttackConfig
    from bimodalattack_amd.config import EngineOptions
    monkeypatch.delenv("BMA_PGD_RULE", raising=False)
    assert EngineOptions.from_env().pgd_rule == "linf"
    assert EngineOptions.from_env(pgd_rule="apgd").pgd_rule == "apgd"
    monkeypatch.setenv("BMA_PGD_RULE", "apgd")
    assert EngineOptions.from_env().pgd_rule == "apgd"
    assert EngineOptions.from_env(pgd_rule="linf").pgd_rule == "linf"          # the keyword wins over the environment
    monkeypatch.setenv("BMA_PGD_RULE", "l2")
    with pytest.raises(ValueError, match="pgd_rule"):
        EngineOptions.from_env()
    monkeypatch.delenv("BMA_PGD_RULE")
    with pytest.raises(ValueError, match="pgd_rule"):
        EngineOptions.from_env(pgd_rule="APGD")
    # an engine option, not a config field: the dataclass stays the reference's 27 fields
    assert len(dataclasses.fields(BimodalAttackConfig)) == 27
    assert "pgd_rule" not in {f.name for f in dataclasses.fields(BimodalAttackConfig)}
