#!/usr/bin/env python3
"""Capture golden vectors G9 -- the reference's ``mellowmax`` (bimodalattack/utils.py:35-36, shipped and never called
there) applied as nanoGCG applies it, to the negated raw target logits -- from the REAL reference, as make_golden.py
captures G1-G7 (same import adapter; numbers only are stored).

    python tests/golden/make_golden_mellowmax.py        # regenerate g9_mellowmax_unit.npz

Per T in {1, 2, 20, 65}: one block of logits (N_CAND, T, V) fp32 whose every value is exact in bfloat16 AND float16, one
label vector, and for alpha in {0.25, 1.0, 4.0} the reference's outputs of ``mellowmax(-gather(logits, labels), alpha)``
on the fp32 input (``out32``) and on the same input in float64 (``out64``).  The candidates (asserted below):

  0-11   ordinary magnitudes (|z| <= 16); candidate 0 carries a NaN and a +inf OFF its label columns (never read)
  12-15  large magnitudes: alpha*t beyond 88 at every alpha, so a sum of exponentials without the maximum taken out overflows
  16     a NaN among the target logits                                   -> NaN
  17     a target logit of -inf (t = +inf)                               -> +inf
  18     every target logit +inf (all t = -inf)                          -> -inf
  19     one target logit +inf among ordinary ones (one t = -inf)        -> finite (for T = 1: -inf)
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import refutils, save  # noqa: E402  (imports the reference, with its adapter stubs)

TS = (1, 2, 20, 65)
ALPHAS = (0.25, 1.0, 4.0)
V = 17
N_CAND = 20


def exact_in_both(a: np.ndarray) -> bool:
    t = torch.from_numpy(a)
    ok = torch.isfinite(t)
    return bool((t.to(torch.bfloat16).float()[ok] == t[ok]).all() and (t.to(torch.float16).float()[ok] == t[ok]).all())


def g9_unit() -> None:
    rs = np.random.RandomState(9)
    out = dict(Ts=np.array(TS, np.int64), alphas=np.array(ALPHAS, np.float64), V=np.int64(V))
    for T in TS:
        # eighths in [-16, 16): at most 8 significant bits, inside float16's range
        z = (rs.randint(-128, 128, size=(N_CAND, T, V)) / 8.0).astype(np.float32)
        labels = rs.randint(0, V, size=T).astype(np.int64)
        labels[0], labels[-1] = 0, V - 1                     # (T = 1: the one label is V - 1)
        j = np.arange(T)
        # 12-15: even integers in [-510, 510]: 0.25 * 352 = 88
        big = (rs.randint(-255, 256, size=(4, T, V)) * 2.0).astype(np.float32)
        big[:, 0, labels[0]] = [-510.0, -400.0, -480.0, -356.0]   # t = 510: alpha*t = 127.5 at the smallest alpha
        z[12:16] = big
        z[16, T // 2, labels[T // 2]] = np.nan
        z[17, T - 1, labels[T - 1]] = -np.inf
        z[18, j, labels] = np.inf
        z[19, 0, labels[0]] = np.inf
        off = (labels[0] + 1) % V                            # off the label column: must never be read
        z[0, 0, off] = np.nan
        z[0, T - 1, (labels[T - 1] + 2) % V] = np.inf
        assert exact_in_both(z)
        out[f"T{T}_logits"], out[f"T{T}_labels"] = z, labels
        zt = torch.from_numpy(z)
        t32 = -zt[:, torch.from_numpy(j), torch.from_numpy(labels)]            # (N_CAND, T)
        for alpha in ALPHAS:
            o32 = refutils.mellowmax(t32, alpha=alpha, dim=-1).numpy()
            o64 = refutils.mellowmax(t32.double(), alpha=alpha, dim=-1).numpy()
            assert o32.dtype == np.float32 and o64.dtype == np.float64
            assert np.isfinite(o64[:16]).all() and (alpha * t32[12:16].numpy().max(axis=1) > 88).all()
            assert np.isnan(o64[16]) and o64[17] == np.inf and o64[18] == -np.inf
            assert np.isfinite(o64[19]) if T > 1 else o64[19] == -np.inf
            with np.errstate(over="ignore"):                 # what the maximum is taken out for
                naive = np.log(np.exp((alpha * t32[12:16].numpy()).astype(np.float32)).sum(-1))
            assert np.isinf(naive).all()
            out[f"T{T}_a{alpha}_out32"], out[f"T{T}_a{alpha}_out64"] = o32, o64
    save("g9_mellowmax_unit.npz", **out)


if __name__ == "__main__":
    torch.set_num_threads(1)  # one reduction order
    g9_unit()
