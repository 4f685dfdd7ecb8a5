"""The float64 references and error bounds of the backward elementwise kernels (oracle/kernels.py: RMSNorm, gated
activation, rotary) on the CPU, without the library: the references against torch float64 autograd through the plain
expressions; the bounds against an fp32 restatement of csrc/fused_elementwise.hip's backward kernels, operation by
operation, which must pass -- and against the same restatement with one deliberate slip, which must not.
tests/test_backward_gpu.py holds the kernels to the same references and bounds."""

import numpy as np
import pytest
import torch

from oracle import kernels as K

from oracle.kernels import NORM_BWD_D as NORM_D, NORM_BWD_EPS as EPS, GATED_BWD_N as GATED_N
from oracle.kernels import gated_bwd_ratios as gated_ratios, norm_bwd_ratio as norm_ratio, rope_inputs, rope_round_trip_tol

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
F32 = torch.float32


def _rnd(v, dt):
    return v.to(dt).to(F32)


# ------------------------------------------------------------------ the kernels, restated in fp32
def restate_rmsnorm_bwd(x, w, dy, eps, gemma, dsum, dt, slip=None):
    """rmsnorm_bwd_kernel: 256 lanes, lane t owns the 16-byte chunks t, t+256, ...; both sums run sequentially in the
    lane, then over the 64 lanes of a wave, then over the four waves; the output is rounded once (twice with dsum)."""
    rows, D = x.shape
    ne = 16 // x.element_size()
    nch = -(-(D // ne) // 256)
    xf, wf, df = x.to(F32), w.to(F32), dy.to(F32)
    one_w = gemma != (slip == "w_swap")
    gf = df * (1.0 + wf if one_w else wf)
    Dd = np.float32(D + 1 if slip == "D+1" else D)

    def lanes(v):                                     # (rows, D) -> (rows, nch, 256, ne), zero beyond the row
        pad = torch.zeros((rows, nch * 256 * ne), dtype=F32)
        pad[:, :D] = v
        return pad.view(rows, nch, 256, ne)

    xl, gl = lanes(xf), lanes(gf)
    ss, sg = torch.zeros((rows, 256)), torch.zeros((rows, 256))
    for c in range(nch):
        for j in range(ne):
            ss = ss + xl[:, c, :, j] * xl[:, c, :, j]
            sg = sg + gl[:, c, :, j] * xl[:, c, :, j]

    def block_sum(v):
        v = v.view(rows, 4, 64)
        h = 32
        while h:
            v = v[..., :h] + v[..., h:2 * h]
            h //= 2
        v = v[..., 0]
        return ((v[:, 0] + v[:, 1]) + v[:, 2]) + v[:, 3]

    tss, tsg = block_sum(ss)[:, None], block_sum(sg)[:, None]
    r = 1.0 / torch.sqrt(tss / Dd + np.float32(eps))
    k = r * r * r * tsg / Dd
    o = r * gf - xf * k
    if dsum is not None and slip != "no_dsum":
        o = dsum.to(F32) + _rnd(o, dt)
    return o.to(dt)


def _fma_kappa(x3, x):
    """fmaf(kappa, x3, x): the exact product and sum, rounded once (float64 holds the 48-bit product exactly)."""
    kappa = torch.tensor(0.044715, dtype=F32).double()
    return (kappa * x3.double() + x.double()).to(F32)


def restate_gated_bwd(gate, up, dy, act, dt, slip=None):
    """swiglu_bwd_kernel's element: (d_gate, d_up), fp32 throughout, the activation rounded to dt before d_up."""
    g, u, d = gate.to(F32), up.to(F32), dy.to(F32)
    if act == 0:
        s = 1.0 / (1.0 + torch.exp(-g))
        a = _rnd(g * s, dt)
        dd = s * (1.0 + g * (s if slip == "g*s" else 1.0 - s))
    else:
        beta, kappa = torch.tensor(0.7978845608028654, dtype=F32), torch.tensor(0.044715, dtype=F32)
        x2 = g * g
        t = torch.tanh(beta * _fma_kappa(x2 * g, g))
        k3 = kappa if slip == "kappa" else 3.0 * kappa
        dd = 0.5 * g * (1.0 - t * t) * (beta * (1.0 + k3 * x2))
        if slip != "no_half":
            dd = 0.5 * (1.0 + t) + dd
        a = _rnd(0.5 * g * (1.0 + t), dt)
    if slip == "d_up_from_up":
        a = u
    return (d * u * dd).to(dt), (d * a).to(dt)


def restate_rope(q, cos, sin, sign, dt):
    """rope_row: rnd(rnd(x*cos) + rnd(sign*partner*sin)), fp32 between the roundings."""
    qf, cf, sf = q.to(F32), cos.to(F32)[:, None], sin.to(F32)[:, None]
    h = q.shape[-1] // 2
    p = torch.cat([qf[..., h:], qf[..., :h]], -1)
    sg = torch.cat([-torch.ones(h), torch.ones(h)]) * np.float32(sign)
    return (_rnd(qf * cf, dt) + _rnd(sg * p * sf, dt)).to(dt)


# ------------------------------------------------------------------ the rounding helper
@pytest.mark.parametrize("dt", DTYPES)
def test_round_dt_is_the_dtype_conversion(dt):
    """round_dt against torch's conversion from fp32 (one rounding) over normal, subnormal, tie and overflowing values,
    and on a float64 tie that a conversion through fp32 would round the wrong way."""
    gen = torch.Generator().manual_seed(5)
    v = torch.randn(200000, generator=gen) * torch.exp2(torch.randint(-150, 130, (200000,), generator=gen).float())
    v = torch.cat([v, torch.tensor([0.0, -0.0, 1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 65504.0, 65520.0, 3.4e38, -3.4e38,
                                    2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -133, 2.0 ** -134, float("inf")])])
    want = v.to(dt).double()
    got = K.round_dt(v.double(), dt)
    assert torch.equal(got, want) and torch.equal(torch.signbit(got), torch.signbit(want))
    if dt != torch.float32:
        p = {torch.bfloat16: 8, torch.float16: 11}[dt]
        tie_up = torch.tensor([1.0 + 2.0 ** -p + 2.0 ** -40], dtype=torch.float64)      # just above the tie 1 + u
        assert K.round_dt(tie_up, dt).item() == 1.0 + 2.0 ** (1 - p)
        assert tie_up.float().to(dt).item() == 1.0                                       # the double rounding it avoids


# ------------------------------------------------------------------ references against float64 autograd
@pytest.mark.parametrize("gemma", [False, True])
def test_rmsnorm_bwd_ref_is_float64_autograd(gemma):
    """x*rsqrt(mean(x^2)+eps)*w (or *(1+w)) under torch float64 autograd: equal to 1e-12 of the uncancelled size
    rg + xk (the one-hot row cancels to 1e-6 of it, so a bound relative to the result itself would be of the noise)."""
    for D in (8, 256, 2560):
        x, w, dy, dsum = (t.double() for t in K.norm_bwd_inputs(6, D, torch.float16, gemma))
        eps = float(np.float32(EPS[gemma]))
        xa = x.clone().requires_grad_()
        y = xa * torch.rsqrt((xa * xa).mean(-1, keepdim=True) + eps) * (1.0 + w if gemma else w)
        (want,) = torch.autograd.grad(y, xa, dy)
        ref = K.rmsnorm_bwd_ref(x, w, dy, EPS[gemma], gemma)
        assert bool(((ref.ref - want).abs() <= 1e-12 * (ref.rg + ref.xk)).all())
        ref2 = K.rmsnorm_bwd_ref(x, w, dy, EPS[gemma], gemma, dsum)
        assert torch.equal(ref2.ref, dsum + ref.dxn) and torch.equal(ref2.dxn, ref.dxn)
        assert bool((ref.rg + ref.xk >= ref.dxn.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("act", [0, 1])
def test_gated_act_bwd_ref_is_float64_autograd(act):
    """F.silu(a)*b and F.gelu(a, approximate="tanh")*b under float64 autograd: activation, d_gate and d_up to 1e-12
    relative (d_gate relative to |dy*up|*(1+|g|...), the size its terms have before they cancel at the zeros of act')."""
    gate, up, dy = (t.double() for t in K.gated_bwd_inputs(65536, torch.float16))
    a, b = gate.clone().requires_grad_(), up.clone().requires_grad_()
    fn = torch.nn.functional.silu if act == 0 else (lambda t: torch.nn.functional.gelu(t, approximate="tanh"))
    ga, gb = torch.autograd.grad(fn(a) * b, (a, b), dy)
    a64, d64, ref = K.gated_act_bwd_ref(gate, up, dy, act)
    m = (dy * up).abs() * (1.0 + gate.abs() * (1.0 + (3 * K.GELU_KAPPA * gate * gate if act else 0.0)))
    assert bool(((ref - ga).abs() <= 1e-12 * m).all())
    assert bool(((dy * a64 - gb).abs() <= 1e-12 * (dy * gate).abs()).all())
    assert bool(((a64 - fn(gate)).abs() <= 1e-12 * gate.abs()).all())
    # the derivative changes sign inside each cluster of gates placed on its zero
    z = K.SILU_DZERO if act == 0 else K.GELU_DZERO
    near = (gate - z).abs() <= 1.1e-2
    assert int(near.sum()) >= 65536 // 8 and bool((d64[near] > 0).any()) and bool((d64[near] < 0).any())


@pytest.mark.parametrize("dt", DTYPES)
def test_rope_ref_is_the_rotation(dt):
    """rope_ref(sign=-1) is float64 autograd's gradient of the plain rotation q*cos + rotate_half(q)*sin to two
    roundings of the dtype per term, and the inverse of rope_ref(sign=+1) to two roundings of the vector's size."""
    u = K.unit_roundoff(dt)
    q, cos, sin, dq = rope_inputs(3, 2, 65, 64, 3, dt)
    qa = q.double().clone().requires_grad_()
    h = 32
    rot = torch.cat([-qa[..., h:], qa[..., :h]], -1)
    (want,) = torch.autograd.grad(qa * cos.double()[:, None] + rot * sin.double()[:, None], qa, dq.double())
    got = K.rope_ref(dq, cos, sin, -1, dt)
    part = torch.cat([dq[..., h:], dq[..., :h]], -1).double().abs()
    assert bool(((got - want).abs() <= 2 * u * (dq.double().abs() + part) + K.half_subnormal(dt)).all())


# ------------------------------------------------------------------ the restated kernels pass the bounds
@pytest.mark.parametrize("dt", DTYPES)
def test_restated_rmsnorm_bwd_passes_the_bound(dt):
    """Every (gemma, dsum, D, rows) of the GPU test.  Worst |error| / bound of the faithful restatement on this CPU:
    bf16 0.994, fp16 0.990 (the result's own rounding; the fp32 evaluation uses 0.06 of its share), fp32 0.863 (with dsum,
    the x*100 row: the rounding of the add), 0.06 without dsum."""
    worst = 0.0
    for gemma in (False, True):
        for D in NORM_D[dt]:
            for rows in (1, 6):
                x, w, dy, dsum = K.norm_bwd_inputs(rows, D, dt, gemma)
                for ds in (None, dsum):
                    got = restate_rmsnorm_bwd(x, w, dy, EPS[gemma], gemma, ds, dt)
                    r = norm_ratio(got, x, w, dy, EPS[gemma], gemma, ds, dt)
                    worst = max(worst, r)
                    assert r <= 1.0, (gemma, D, rows, ds is not None, r)
    print(f"rmsnorm_bwd restated {dt}: worst ratio {worst:.3f}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("act", [0, 1])
def test_restated_gated_bwd_passes_the_bounds(dt, act):
    """n = 8, 24 and 65,536.  Worst ratios of the faithful restatement on this CPU (d_gate error / bound; d_up distance
    from the interval's centre / half-width) and the share of elements whose activation may round either way:
        SiLU  bf16 0.995 / 0.988 / 0.15 %    fp16 0.991 / 0.999 / 0.05 %    fp32 0.131 / 0.397 / -
        GELU  bf16 0.990 / 0.988 / 17.9 %    fp16 0.995 / 0.987 / 20.7 %    fp32 0.104 / 0.224 / -
    (in the 16-bit types the ratio is the result's own rounding, a uniform error reaching its half-spacing).
    The share is a condition for the 16-bit types at n = 65,536: at most 1 % (SiLU) and 25 % (GELU)."""
    for n in GATED_N:
        gate, up, dy = K.gated_bwd_inputs(n, dt)
        dg, du = restate_gated_bwd(gate, up, dy, act, dt)
        rg, ru, share = gated_ratios(dg, du, gate, up, dy, act, dt)
        print(f"gated_bwd restated {dt} act={act} n={n}: d_gate {rg:.3f} d_up {ru:.3f} ambiguous {share:.4f}")
        assert rg <= 1.0 and ru <= 1.0, (n, rg, ru)
        if n == 65536 and dt != torch.float32:
            assert share <= (0.01 if act == 0 else 0.25), share


@pytest.mark.parametrize("dt", DTYPES)
def test_restated_rope_is_rope_ref_bit_for_bit(dt):
    for Dh in (64, 128, 256):
        for L in (1, 65):
            for cb in (1, 3):
                q, cos, sin, dq = rope_inputs(3, 2, L, Dh, cb, dt)
                for sign, src in ((1, q), (-1, dq)):
                    got = restate_rope(src, cos, sin, sign, dt)
                    assert torch.equal(got.double(), K.rope_ref(src, cos, sin, sign, dt)), (Dh, L, cb, sign)
                back = K.rope_ref(K.rope_ref(q, cos, sin, 1, dt), cos, sin, -1, dt)
                assert bool(((back - q.double()).abs() <= rope_round_trip_tol(q, dt)).all()), (Dh, L, cb)


# ------------------------------------------------------------------ one slip each: the bounds reject it
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("slip", ["w_swap", "D+1", "no_dsum"])
def test_bound_rejects_a_slip_in_rmsnorm_bwd(dt, slip):
    """w for 1+w (and back), D+1 for D (claimed at D <= 2560 only: beyond, the change is below one 16-bit rounding),
    the residual-stream gradient dropped."""
    for gemma in (False, True):
        for D in [d for d in NORM_D[dt] if slip != "D+1" or d <= 2560]:
            x, w, dy, dsum = K.norm_bwd_inputs(6, D, dt, gemma)
            ds = dsum if slip == "no_dsum" else None
            got = restate_rmsnorm_bwd(x, w, dy, EPS[gemma], gemma, ds, dt, slip=slip)
            assert norm_ratio(got, x, w, dy, EPS[gemma], gemma, ds, dt) > 1.0, (gemma, D)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("act,slip", [(0, "g*s"), (1, "kappa"), (1, "no_half"), (0, "d_up_from_up"), (1, "d_up_from_up")])
def test_bound_rejects_a_slip_in_gated_bwd(dt, act, slip):
    """s*(1+g*s) for s*(1+g*(1-s)); GELU' with kappa for 3*kappa; GELU' without 0.5*(1+t); d_up from up."""
    gate, up, dy = K.gated_bwd_inputs(65536, dt)
    dg, du = restate_gated_bwd(gate, up, dy, act, dt, slip=slip)
    rg, ru, _ = gated_ratios(dg, du, gate, up, dy, act, dt)
    assert (ru if slip == "d_up_from_up" else rg) > 1.0, (rg, ru)
    good = restate_gated_bwd(gate, up, dy, act, dt)
    assert torch.equal(good[1] if slip != "d_up_from_up" else good[0], du if slip != "d_up_from_up" else dg)


@pytest.mark.parametrize("dt", DTYPES)
def test_rope_ref_rejects_plus_sin_in_the_inverse(dt):
    q, cos, sin, dq = rope_inputs(3, 2, 65, 128, 3, dt)
    assert not torch.equal(restate_rope(dq, cos, sin, 1, dt).double(), K.rope_ref(dq, cos, sin, -1, dt))
