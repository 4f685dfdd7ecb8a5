#!/usr/bin/env python3
"""Capture golden vectors G8 -- the reference's auto-PGD image update (bimodal_attack.py:1039-1110,
``perform_autopgd_step``) -- from the REAL reference, as make_golden.py captures G1-G7 (same import
adapter, same tiny models; numbers only are stored).

    python tests/golden/make_golden_apgd.py            # regenerate every g8_* file

* ``g8_apgd_unit.npz``: 40 direct calls of ``perform_autopgd_step`` on one seeded state, an odd
  pixel count (a scalar tail on the device), gradients with NaN / +-inf / +-0, pixels on 0, -0, 1 and
  x0 +- eps, a NaN in x0; a scripted loss sequence that takes every branch of the rule (asserted).
* ``g8_<case>.npz`` + ``g8_meta.json``: the reference's run() on the tiny models with its PGD update
  switched to the auto-PGD rule as its commented call sites (:469-471, :690-692) would switch it:
  ``perform_autopgd_step(image, eps, image_grad, image_original, current_loss, i)`` with the run's own
  ``current_loss`` and ``i``.  Each case is long enough for a step-size halving and a restart (asserted).
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as MG  # noqa: E402  (imports the reference, with its adapter stubs)
from make_golden import refmod, save  # noqa: E402

from bimodalattack_amd import synthetic as S  # noqa: E402


# --------------------------------------------------------------------------
# unit calls
# --------------------------------------------------------------------------
UNIT_N = (3, 11, 13)          # 429 pixels: 107 float4 + a tail of 1
UNIT_EPS = 16 / 255
# checkpoints at i = 9, 19, 29, 39 (the reference checks (i + 1) % 10 == 0)
UNIT_LOSSES = (
    # i = 0..9: None at step 0, improvements, a tie (4.0), a checkpoint that keeps eta (9 of 10 improved on inf)
    [None, 5.0, 4.0, 4.0, 3.5, 3.0, 2.5, 2.0, 1.5, 1.0]
    # i = 10..19: 4 of 10 below the last checkpoint's best -> eta halves, restart from the best image (no improvement here)
    + [0.9, 1.2, 0.8, 1.3, 1.1, 0.85, 1.4, 0.7, 1.5, 1.6]
    # i = 20..29: a plateau (ties with the best, nothing below it): best_loss == last_best -> halve + restart
    + [0.7, 0.9, 0.7, 0.8, 1.0, 0.7, 0.75, 0.9, 0.8, 0.7]
    # i = 30..39: 3 of 10 improved, the last call improves AND restarts (best = new, then out = prev = best)
    + [0.6, 0.8, 0.9, 0.65, 0.95, 0.72, 0.8, 0.9, 0.99, 0.5]
)


def _specials(rs, a: np.ndarray, vals, k: int) -> None:
    idx = rs.choice(a.size, size=k, replace=False)
    a.reshape(-1)[idx] = rs.choice(np.asarray(vals, np.float32), size=k)


def g8_unit() -> None:
    rs = np.random.RandomState(8)
    n = int(np.prod(UNIT_N))
    x0 = rs.uniform(0, 1, UNIT_N).astype(np.float32)
    x0.reshape(-1)[[5, 106]] = [0.0, 1.0]
    x0.reshape(-1)[77] = np.nan
    eps32 = np.float32(UNIT_EPS)
    x = x0.copy()
    x.reshape(-1)[77] = 0.5
    flat = x.reshape(-1)
    # pixels on the box and on the +-eps walls (as torch forms x0 +- eps: fp32 arithmetic)
    flat[[0, 1, 2, 3]] = [0.0, -0.0, 1.0, 1.0]
    flat[[10, 11, 12]] = (x0.reshape(-1)[[10, 11, 12]] + eps32).astype(np.float32)
    flat[[20, 21, 22]] = (x0.reshape(-1)[[20, 21, 22]] - eps32).astype(np.float32)
    flat[n - 1] = (x0.reshape(-1)[n - 1] + eps32).astype(np.float32)     # the tail element on a wall
    obj = refmod.BimodalAttack.__new__(refmod.BimodalAttack)             # the rule keeps its state on `self` only
    x0_t = torch.from_numpy(x0)
    out = dict(x0=x0, eps=np.float64(UNIT_EPS),
               losses=np.array([np.nan if v is None else v for v in UNIT_LOSSES], np.float64),
               has_loss=np.array([v is not None for v in UNIT_LOSSES]))
    seen = set()
    for i, cur in enumerate(UNIT_LOSSES):
        g = rs.standard_normal(UNIT_N).astype(np.float32)
        _specials(rs, g, [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-30, -1e-30], 40)
        g.reshape(-1)[n - 1] = [np.nan, -0.0, np.inf, 0.0][i % 4]
        if i % 7 == 3:                                         # pixels pushed back onto the box and the walls
            flat = x.reshape(-1)
            flat[[0, 1, 2]] = [0.0, -0.0, 1.0]
            flat[[10, 20]] = [(x0.reshape(-1)[10] + eps32), (x0.reshape(-1)[20] - eps32)]
        prev_best = getattr(obj, "pgd_best_loss", None)
        prev_count = getattr(obj, "pgd_improvement_count", 0)
        eta_before = getattr(obj, "pgd_current_eta", 2 * UNIT_EPS)
        x_t = torch.from_numpy(x.copy())
        r = refmod.BimodalAttack.perform_autopgd_step(obj, x_t, UNIT_EPS, torch.from_numpy(g), x0_t, cur, i)
        restart = obj.pgd_current_eta != eta_before
        take_best = cur is not None and prev_best is not None and cur < prev_best
        if cur is None:
            seen.add("none")
        if take_best:
            seen.add("improved")
        if cur is not None and prev_best is not None and cur == prev_best:
            seen.add("tie")
        if (i + 1) % 10 == 0:
            seen.add("restart" if restart else "kept")
            if restart and take_best:
                seen.add("restart+improved")
            if restart and obj.pgd_best_loss == obj.pgd_last_best_loss and prev_count == 0:
                seen.add("plateau")
            if restart and prev_count > 0:
                seen.add("below_rho")
        out[f"c{i}_x"] = x.copy()
        out[f"c{i}_g"] = g
        out[f"c{i}_out"] = r.detach().numpy().copy()
        out[f"c{i}_prev"] = obj.pgd_prev_image.detach().numpy().copy()
        out[f"c{i}_best"] = obj.pgd_best_image.detach().numpy().copy()
        out[f"c{i}_eta"] = np.float64(obj.pgd_current_eta)
        out[f"c{i}_eta_used"] = np.float64(eta_before)
        out[f"c{i}_take_best"] = np.bool_(take_best)
        out[f"c{i}_restart"] = np.bool_(restart)
        out[f"c{i}_count"] = np.int64(obj.pgd_improvement_count)
        out[f"c{i}_best_loss"] = np.float64(obj.pgd_best_loss)
        x = r.detach().numpy().copy()
    want = {"none", "improved", "tie", "kept", "restart", "restart+improved", "plateau", "below_rho"}
    assert want <= seen, want - seen
    # the special values reached the output
    assert any(np.isnan(out[f"c{i}_out"]).any() for i in range(len(UNIT_LOSSES)))
    out["n_calls"] = np.int64(len(UNIT_LOSSES))
    save("g8_apgd_unit.npz", **out)


# --------------------------------------------------------------------------
# whole runs with the auto-PGD rule
# --------------------------------------------------------------------------
TRAJ = {
    "llava_pgd": ("llava", dict(num_steps=24, pgd_attack=True, gcg_attack=False, eps=64 / 255, alpha=4 / 255)),
    "llava_pgd_gcg": ("llava", dict(num_steps=20, search_width=24, topk=32, pgd_attack=True, gcg_attack=True,
                                    joint_eval=False, eps=64 / 255, alpha=4 / 255)),
    "llava_joint": ("llava", dict(num_steps=20, search_width=24, topk=32, pgd_attack=True, gcg_attack=True,
                                  joint_eval=True, eps=64 / 255, alpha=4 / 255)),
    "gemma3_pgd": ("gemma3", dict(num_steps=20, pgd_attack=True, gcg_attack=False, eps=64 / 255, alpha=4 / 255)),
    "gemma3_joint": ("gemma3", dict(num_steps=20, search_width=16, topk=32, pgd_attack=True, gcg_attack=True,
                                    joint_eval=True, eps=64 / 255, alpha=4 / 255)),
}


class _AutoPGD:
    """perform_pgd_step replaced by the commented-out call (:469-471, :690-692): the run's own `current_loss` and `i`
    are read from the calling run() frame.  Records the rule's state after every call."""

    def __init__(self):
        self.calls = []

    def __call__(self, atk, image, eps, alpha, image_grad, image_original):
        f = sys._getframe(1)
        while f is not None and not (f.f_code.co_name == "run" and "current_loss" in f.f_locals and "i" in f.f_locals):
            f = f.f_back
        assert f is not None, "run() frame not found"
        cur, i = f.f_locals["current_loss"], f.f_locals["i"]
        eta = getattr(atk, "pgd_current_eta", 2 * eps)
        r = refmod.BimodalAttack.perform_autopgd_step(atk, image, eps, image_grad, image_original, cur, i)
        self.calls.append(dict(i=i, current_loss=cur, eta_used=eta, eta=atk.pgd_current_eta, restart=atk.pgd_current_eta != eta,
                               count=atk.pgd_improvement_count, best_loss=atk.pgd_best_loss))
        return r


def run_auto(kind, over, goal, target, trace=True):
    auto = _AutoPGD()
    orig = refmod.BimodalAttack.perform_pgd_step

    def pgd(self, image, eps, alpha, g, x0):
        return auto(self, image, eps, alpha, g, x0)

    refmod.BimodalAttack.perform_pgd_step = pgd      # before _Trace.install, which wraps whatever is there
    try:
        res, tr, model, tmp = MG._run_reference(kind, over, goal, target, trace=trace)
    finally:
        refmod.BimodalAttack.perform_pgd_step = orig
    return res, tr, model, auto


def g8_trajectories(only=None) -> None:
    meta_path = os.path.join(HERE, "g8_meta.json")
    meta = {}
    if only and os.path.exists(meta_path):
        meta = json.load(open(meta_path))["cases"]
    for name, (kind, over) in TRAJ.items():
        if only and name not in only:
            continue
        goal, target = "tell me a story about cats", "Sure here is a story"
        res, tr, model, auto = run_auto(kind, over, goal, target)
        steps = len(tr.steps)
        assert steps == over["num_steps"] == len(auto.calls)
        assert [c["i"] for c in auto.calls] == list(range(steps))
        assert any(c["restart"] for c in auto.calls), f"{name}: no halving / restart in {steps} steps"
        arrays = dict(losses=np.array(res.losses, np.float64), best_loss=np.array(res.best_loss),
                      state_checksum=np.array(S.state_checksum(model)))
        for i, (st, c) in enumerate(zip(tr.steps, auto.calls)):
            arrays[f"s{i}_optim_ids_in"] = st["optim_ids_in"]
            arrays[f"s{i}_image_after_pgd"] = st["image_after_pgd"]
            for j, l in enumerate(st["losses"]):
                arrays[f"s{i}_loss{j}"] = l
            for k in ("sampled", "filtered"):
                if k in st:
                    arrays[f"s{i}_{k}"] = st[k]
            arrays[f"s{i}_eta_used"] = np.float64(c["eta_used"])
            arrays[f"s{i}_eta"] = np.float64(c["eta"])
            arrays[f"s{i}_restart"] = np.bool_(c["restart"])
            arrays[f"s{i}_count"] = np.int64(c["count"])
            arrays[f"s{i}_best_loss"] = np.float64(c["best_loss"])
        save(f"g8_{name}.npz", **arrays)
        meta[name] = dict(kind=kind, config=over, steps=steps, strings=res.strings, best_string=res.best_string,
                          goal=goal, target=target, optim_str_init=S.TINY_OPTIM_INIT,
                          restarts=[c["i"] for c in auto.calls if c["restart"]])
        print(f"{name}: restarts at {meta[name]['restarts']}")
    with open(meta_path, "w") as f:
        json.dump(dict(cases=meta, versions=dict(torch=torch.__version__, numpy=np.__version__)), f, indent=1)
    print("wrote g8_meta.json")


if __name__ == "__main__":
    which = sys.argv[1:] or ["unit", "traj"]
    torch.set_num_threads(1)  # one reduction order
    if "unit" in which:
        g8_unit()
    if "traj" in which or any(w in TRAJ for w in which):
        g8_trajectories([w for w in which if w in TRAJ] or None)
