"""The float64 references and per-element error bounds of the gradient-pass attention kernels (oracle/kernels.py:
attention_ref, b1_attention_ref) on the CPU, without the library: the references against torch float64 autograd through
the plain expression; the bounds against fp32 restatements of csrc/causal_attention.hip and csrc/b1_attention.hip that
follow the kernels' own rounding points, which must pass -- and against the same restatements with one deliberate slip,
which must not.  The restatements over the whole case matrix are also where K.ATTN_C and K.ATTN_C_LSE come from.
tests/test_attention_grad_gpu.py holds the kernels to the same references and bounds."""

import functools
import math

import pytest
import torch

from oracle import kernels as K
from oracle.kernels import AttnCase

DTYPES = [torch.bfloat16, torch.float16]
F32 = torch.float32
NEG = float("-inf")


def _rnd(v, dt):
    return v.to(dt).to(F32)


def _fma(a, b, c):
    """fmaf(a, b, c) with b a scalar: the product is exact in float64, one rounding of the sum (and a harmless second)."""
    return (a.double() * float(b) + c.double()).to(F32)


def _f32(x):
    return torch.tensor(x, dtype=F32)


# ------------------------------------------------------------------ csrc/causal_attention.hip, restated in fp32
def _mask(Lq, Lk, causal, slip):
    """(Lq, Lk) visibility as the three kernels' `edge` tests leave it, with the slips that live in the mask."""
    P = Lk - Lq
    if slip == "no_offset":                                       # the Lk - Lq offset dropped
        P = 0
    i, j = torch.arange(Lq)[:, None], torch.arange(Lk)[None, :]
    vis = (j <= P + i) if causal else torch.ones((Lq, Lk), dtype=torch.bool)
    blk = (i // 64) == max(Lq - 2, 0) // 64                      # the last 64-query block of more than one row
    if slip == "hide_chunk_key":                                  # the last key of a 32-key chunk, hidden from one block
        n_full = (P + 64 * (max(Lq - 2, 0) // 64) + 1) // 32      # whole chunks the block's first row sees
        vis = vis & ~(blk & (j == 32 * (n_full // 2) + 31))       # the one in the middle
    if slip == "shift_block":                                     # one key past the diagonal for one block
        vis = vis | (blk & (j == P + i + 1))
    if slip == "shift_row":                                       # the same for a single query
        vis = vis | ((i == Lq // 2) & (j == P + i + 1))
    return vis


def restate_causal(q, k, v, d_out, scale, causal, dt, slip=None):
    """causal_fwd_kernel, causal_dq_kernel and causal_dkv_kernel.  Forward: the two wave halves walk the even and the odd
    32-key chunks with their own online softmax (running maximum of the raw scores, exp2 of fma(s, scale*log2e, -m*..),
    the unnormalised P packed to the 16-bit type before P.V, the accumulator rescaled by alpha); their (m, l, o) meet
    once, o is scaled by a_half / l and rounded once.  dq: delta from the ROUNDED o, P = exp2(fma(s, .., -lse2)),
    dS = P (dP - delta) scale rounded before dS.K, the halves' sums added, one rounding.  dk / dv: per 32-query chunk P
    and dS rounded before P^T.dO and dS^T.Q, the halves take the even and the odd query chunks over every head of the
    group, fp32 sums, one rounding.  Returns {o, lse2, dq, dk, dv} in the kernels' types."""
    (Lq, H, Dh), (Lk, Hkv, _) = q.shape, k.shape
    rep = H // Hkv
    qf, dof = q.to(F32).transpose(0, 1), d_out.to(F32).transpose(0, 1)                    # (H, Lq, Dh)
    kf = k.to(F32).repeat_interleave(rep, 1).transpose(0, 1)                                 # (H, Lk, Dh)
    vf = v.to(F32).repeat_interleave(rep, 1).transpose(0, 1)
    sc, sl2e = _f32(scale), _f32(scale) * _f32(1.4426950408889634)
    vis = _mask(Lq, Lk, causal, slip)
    s = (qf @ kf.transpose(1, 2)).masked_fill(~vis[None], NEG)                             # raw scores, -inf where hidden
    nch = (Lk + 31) // 32

    halves = []
    for half in (0, 1):
        m, l, acc = torch.full((H, Lq), NEG), torch.zeros((H, Lq)), torch.zeros((H, Lq, Dh))
        for c in range(half, nch, 2):
            sch = s[..., 32 * c:32 * c + 32]
            mnew = torch.maximum(m, sch.amax(-1))
            msafe = torch.where(mnew > NEG, mnew, torch.zeros_like(mnew))
            alpha = torch.exp2((m - msafe) * sl2e)
            e = torch.exp2(_fma(sch, sl2e, (-msafe * sl2e)[..., None].expand_as(sch)))
            l = l * alpha + e.sum(-1)
            acc = acc * alpha[..., None] + _rnd(e, dt) @ vf[:, 32 * c:32 * c + 32]
            m = mnew
        halves.append((m, l, acc))
    (m1, l1, o1), (m2, l2, o2) = halves
    m = torch.maximum(m1, m2)
    a1, a2 = torch.exp2((m1 - m) * sl2e), torch.exp2((m2 - m) * sl2e)
    l = l1 * a1 if slip == "no_renorm" else l1 * a1 + l2 * a2
    inv = 1.0 / l
    lse2 = m * sl2e + torch.log2(l1 * a1 + l2 * a2)
    o = (o1 * (a1 * inv)[..., None] + o2 * (a2 * inv)[..., None]).to(dt)                  # (H, Lq, Dh)

    delta = (dof * o.to(F32)).sum(-1)                                                      # (H, Lq)
    if slip == "no_delta":
        delta = torch.zeros_like(delta)
    if slip == "delta_wrong_head":
        delta = delta.roll(1, 0)
    p = torch.exp2(_fma(s, sl2e, (-lse2)[..., None].expand_as(s)))                         # exp2(-inf) = 0 where hidden
    dp = dof @ vf.transpose(1, 2)
    ds = p * (dp - delta[..., None])
    if slip != "no_scale":
        ds = ds * sc
    p16, ds16 = _rnd(p, dt), _rnd(ds, dt)
    dq = torch.zeros((2, H, Lq, Dh))
    for c in range(nch):
        dq[c & 1] += ds16[..., 32 * c:32 * c + 32] @ kf[:, 32 * c:32 * c + 32]
    dq = (dq[0] + dq[1]).to(dt)

    dk, dv = torch.zeros((2, Hkv, Lk, Dh)), torch.zeros((2, Hkv, Lk, Dh))
    split_d = Dh > 128                                            # 256-wide heads: every wave walks every chunk
    for g in range(1 if slip == "group_first_head" else rep):
        hs = slice(g, H, rep)                                     # head g of every group
        for c in range((Lq + 31) // 32):
            rows = slice(32 * c, 32 * c + 32)
            half = 0 if split_d else c & 1
            dv[half] += p16[hs, rows].transpose(1, 2) @ dof[hs, rows]
            dk[half] += ds16[hs, rows].transpose(1, 2) @ qf[hs, rows]
    t = lambda x: x.transpose(0, 1).contiguous()      # noqa: E731
    return {"o": t(o), "lse2": lse2, "dq": t(dq), "dk": t((dk[0] + dk[1]).to(dt)), "dv": t((dv[0] + dv[1]).to(dt))}


# ------------------------------------------------------------------ csrc/b1_attention.hip, restated in fp32
def _rope32(x, cos, sin, sign, dt):
    """rope_regs: rnd(rnd(x cos) + rnd(+-x' sin)) on x (S, H, 128), fp32 between the roundings."""
    h = x.shape[-1] // 2
    xf, cf, sf = x.to(F32), cos.to(F32)[:, None], sin.to(F32)[:, None]
    part = torch.cat([xf[..., h:], xf[..., :h]], -1)
    sg = torch.cat([-torch.ones(h), torch.ones(h)]) * sign
    return _rnd(_rnd(xf * cf, dt) + _rnd(sg * part * sf, dt), dt)


def restate_b1(qkv, cos, sin, H, scale, d_out, dt, slip=None):
    """b1_attn_fwd_kernel and b1_attn_bwd_kernel: q and k rotated in the 16-bit type; forward: scores times scale, their
    maximum, expf, the NORMALISED P rounded before P.V, one rounding of o, lse = m + log(l); backward: delta from the
    rounded o, P = expf(s scale - lse) and dS = P (dP - delta) scale each rounded before their products, dq' / dk' / dv
    rounded, the inverse rotation of the rounded dq' / dk' with bma_rope2's three roundings.  {o, lse, dqkv}."""
    S = qkv.shape[0]
    q, k, v = (t.reshape(S, H, 128) for t in qkv.split(H * 128, dim=-1))
    qr, kr = _rope32(q, cos, sin, 1.0, dt).transpose(0, 1), _rope32(k, cos, sin, 1.0, dt).transpose(0, 1)      # (H, S, 128)
    vf, gf = v.to(F32).transpose(0, 1), d_out.reshape(S, H, 128).to(F32).transpose(0, 1)
    sc = _f32(scale)
    tril = torch.tril(torch.ones((S, S), dtype=torch.bool))
    s = ((qr @ kr.transpose(1, 2)) * sc).masked_fill(~tril, NEG)
    m = s.amax(-1)
    e = torch.exp(s - m[..., None])
    l = e.sum(-1)
    o = (_rnd(e * (1.0 / l)[..., None], dt) @ vf).to(dt)
    lse = m + torch.log(l)
    delta = (gf * o.to(F32)).sum(-1)
    p = torch.exp(s - lse[..., None])
    ds = _rnd(p * (gf @ vf.transpose(1, 2) - delta[..., None]) * sc, dt)
    dv = (_rnd(p, dt).transpose(1, 2) @ gf).to(dt)
    dk = (ds.transpose(1, 2) @ qr).to(dt).transpose(0, 1)                                  # (S, H, 128), rounded
    dq = (ds @ kr).to(dt).transpose(0, 1)
    back = 1.0 if slip == "plus_sin" else -1.0
    dq, dk = _rope32(dq, cos, sin, back, dt).to(dt), _rope32(dk, cos, sin, back, dt).to(dt)
    flat = lambda x: x.reshape(S, H * 128)      # noqa: E731
    return {"o": flat(o.transpose(0, 1)), "lse": lse, "dqkv": torch.cat([flat(dq), flat(dk), flat(dv.transpose(0, 1))], -1)}


# ------------------------------------------------------------------ the references against autograd
@pytest.mark.parametrize("case", [AttnCase(33, 98, 4, 2, 64, True), AttnCase(20, 20, 4, 1, 64, True), AttnCase(17, 40, 2, 2, 64, False)])
def test_attention_ref_is_autograd_of_the_plain_expression(case):
    """attention_ref's o, lse2, dq, dk, dv against float64 autograd through softmax(q k^T scale + mask) v with the
    keys and values repeated over the group (autograd doing the group's sum), behind a prefix."""
    q, k, v, do = K.attention_inputs(case, torch.bfloat16, "randn")
    rep, scale = case.H // case.Hkv, float(torch.tensor(case.Dh ** -0.5, dtype=F32))
    ref = K.attention_ref(q, k, v, do, scale, case.causal, torch.bfloat16)
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    s = torch.einsum("qhd,khd->hqk", qd, kd.repeat_interleave(rep, 1)) * scale
    if case.causal:
        hidden = torch.arange(case.Lk)[None, :] > (case.Lk - case.Lq + torch.arange(case.Lq))[:, None]
        s = s.masked_fill(hidden[None], NEG)
    o = torch.einsum("hqk,khd->qhd", s.softmax(-1), vd.repeat_interleave(rep, 1))
    gq, gk, gv = torch.autograd.grad(o, (qd, kd, vd), do.double())
    for got, want in ((ref.o, o.detach()), (ref.dq, gq), (ref.dk, gk), (ref.dv, gv),
                      (ref.lse2, torch.logsumexp(s.detach(), -1) / math.log(2.0))):
        assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    for name in ("o", "dq", "dk", "dv"):                        # the bounds are sums of sizes: they dominate the sums themselves
        assert bool((ref.B[name] >= getattr(ref, name).abs() * (1 - 1e-12)).all())
        assert ref.B[name].shape == ref.Z[name].shape == getattr(ref, name).shape and bool((ref.Z[name] >= ref.B[name] * (1 - 1e-12)).all())


def test_b1_attention_ref_is_autograd_through_the_rotation():
    """b1_attention_ref's dqkv against float64 autograd through rotation + attention, where the reference's rounding of
    the rotated q and k is passed through as if it were the identity (straight-through): the difference is then only
    what those two roundings move, far below the bound; and exactly autograd when the rotation is the identity."""
    S, H, dt = 19, 3, torch.float16
    for identity in (True, False):
        qkv, cos, sin, do = K.b1_inputs(S, H, dt, "randn")
        if identity:
            cos, sin = torch.ones_like(cos), torch.zeros_like(sin)
        scale = float(torch.tensor(128 ** -0.5, dtype=F32))                                # the reference takes the fp32 number
        ref = K.b1_attention_ref(qkv, cos, sin, H, scale, do, dt)
        leaf = qkv.double().requires_grad_()
        q, k, v = (t.reshape(S, H, 128) for t in leaf.split(H * 128, dim=-1))
        c, s_ = cos.double()[:, None], sin.double()[:, None]

        def rot(x):
            y = x * c + torch.cat([-x[..., 64:], x[..., :64]], -1) * s_
            return y + (K.round_dt(y.detach(), dt) - y.detach())                          # straight-through rounding
        s = torch.einsum("qhd,khd->hqk", rot(q), rot(k)) * scale
        s = s.masked_fill(~torch.tril(torch.ones((S, S), dtype=torch.bool)), NEG)
        o = torch.einsum("hqk,khd->qhd", s.softmax(-1), v).reshape(S, H * 128)
        (grad,) = torch.autograd.grad(o, leaf, do.double())
        lse = torch.logsumexp(s.detach(), -1)
        if identity:
            assert float((ref.dqkv - grad).abs().max()) <= 1e-12 * float(grad.abs().max())
            assert float((ref.o - o.detach()).abs().max()) <= 1e-12 and float((ref.lse - lse).abs().max()) <= 1e-12
        else:
            # rope_ref rounds the two products as well: the rotated operands differ from the straight-through ones by
            # roundings of `dt`, which the bound (made for a kernel that rounds P and dS) covers many times over
            assert bool(((ref.dqkv - grad).abs() <= ref.tol_dqkv).all()) and bool(((ref.o - o.detach()).abs() <= ref.tol_o).all())
        assert ref.dqkv.shape == ref.tol_dqkv.shape == (S, 3 * H * 128) and ref.lse.shape == (H, S)


# ------------------------------------------------------------------ the bounds against the restatements
@functools.lru_cache(maxsize=None)
def _causal_case(case, dt, family):
    q, k, v, do = K.attention_inputs(case, dt, family)
    return q, k, v, do, K.attention_ref(q, k, v, do, case.Dh ** -0.5, case.causal, dt)


def _causal_ratios(case, dt, family, slip=None):
    q, k, v, do, ref = _causal_case(case, dt, family)
    return K.attention_ratios(restate_causal(q, k, v, do, case.Dh ** -0.5, case.causal, dt, slip), ref, dt)


@functools.lru_cache(maxsize=None)
def _b1_case(S, H, dt, family):
    qkv, cos, sin, do = K.b1_inputs(S, H, dt, family)
    return qkv, cos, sin, do, K.b1_attention_ref(qkv, cos, sin, H, 128 ** -0.5, do, dt)


def _b1_ratios(S, H, dt, family, slip=None):
    qkv, cos, sin, do, ref = _b1_case(S, H, dt, family)
    return K.b1_attention_ratios(restate_b1(qkv, cos, sin, H, 128 ** -0.5, do, dt, slip), ref)


@pytest.mark.parametrize("dt", DTYPES)
def test_correct_restatements_pass_and_fix_the_constants(dt):
    """The correct restatements over every case of the GPU tests, all input families: every ratio <= 1 with the fixed
    constants; and the constants are what the procedure gives -- the smallest power of two at least twice the worst
    ratio at C = 1 (K.ATTN_WORST, K.ATTN_LSE_WORST record the measurement over both dtypes)."""
    worst, worst_lse, where = 0.0, 0.0, None
    c_keep, cl_keep = K.ATTN_C, K.ATTN_C_LSE
    for at_one in (True, False):
        if at_one:
            K.ATTN_C = K.ATTN_C_LSE = 1
        try:
            for family in K.ATTN_FAMILIES:
                runs = [(c, _causal_ratios(c, dt, family)) for c in K.attention_cases() + K.ATTN_TWO_TILE_CASES]
                runs += [((S, H), _b1_ratios(S, H, dt, family)) for S in K.B1_S for H in K.B1_H]
                for case, rs in runs:
                    for name, (r, el) in rs.items():
                        if at_one and name in ("lse2", "lse"):
                            worst_lse = max(worst_lse, r)
                        elif at_one and r > worst:
                            worst, where = r, (case, family, name, el)
                        elif not at_one:
                            assert r <= 1.0, (case, family, name, r, el)
        finally:
            K.ATTN_C, K.ATTN_C_LSE = c_keep, cl_keep
    print(f"restatements {dt}: worst error/bound at C = 1: {worst:.3f} at {where}; lse {worst_lse:.3f}")
    pow2 = lambda x: 2.0 ** math.ceil(math.log2(2.0 * x))      # noqa: E731
    assert worst <= K.ATTN_WORST and worst_lse <= K.ATTN_LSE_WORST
    assert K.ATTN_C == pow2(K.ATTN_WORST) and K.ATTN_C_LSE == pow2(K.ATTN_LSE_WORST)


# every mutant on cases where it can touch something: two workgroups of queries, a prefix, grouped heads; flat and sharp
_MUTANT_CASES = [AttnCase(129, 129, 2, 2, 128, True), AttnCase(65, 200, 2, 2, 128, True), AttnCase(129, 129, 4, 2, 128, True)]
_MUTANTS = [("hide_chunk_key", "o dq dk dv", _MUTANT_CASES),
            ("shift_block", "o dq dk dv", _MUTANT_CASES),
            ("shift_row", "dk dv", _MUTANT_CASES),               # (flat inputs only: under a sharp softmax ONE leaked key may weigh nothing)
            ("no_offset", "o dq dk dv", [AttnCase(20, 84, 2, 2, 128, True), AttnCase(65, 200, 2, 2, 128, True)]),
            ("no_delta", "dq dk", _MUTANT_CASES),
            ("delta_wrong_head", "dq dk", _MUTANT_CASES),
            ("group_first_head", "dk dv", [AttnCase(129, 129, 4, 2, 128, True), AttnCase(65, 200, 4, 1, 128, True)]),
            ("no_scale", "dq dk", _MUTANT_CASES),
            ("no_renorm", "o", _MUTANT_CASES)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("slip,outputs,cases", _MUTANTS, ids=[m[0] for m in _MUTANTS])
def test_a_slip_in_the_causal_restatement_exceeds_the_bound(slip, outputs, cases, dt):
    """One deliberate slip at a time, applied to every row it can touch, on flat and on sharp inputs: each output named
    must leave its bound."""
    for case in cases:
        for family in ("randn",) if slip == "shift_row" else ("randn", "sharp"):
            rs = _causal_ratios(case, dt, family, slip)
            print(f"{slip} {dt} {tuple(case)} {family}: " + " ".join(f"{n}={rs[n][0]:.3g}" for n in ("o", "dq", "dk", "dv")))
            for name in outputs.split():
                assert rs[name][0] > 1.0, (slip, case, family, name, rs[name])


@pytest.mark.parametrize("dt", DTYPES)
def test_b1_inverse_rotation_with_the_wrong_sign_exceeds_the_bound(dt):
    for S, H in ((33, 3), (80, 1)):
        for family in ("randn", "sharp"):
            qkv, cos, sin, do, ref = _b1_case(S, H, dt, family)
            tol, err = ref.tol_dqkv, (restate_b1(qkv, cos, sin, H, 128 ** -0.5, do, dt, "plus_sin")["dqkv"].double() - ref.dqkv).abs()
            for name, cols in (("dq", slice(0, H * 128)), ("dk", slice(H * 128, 2 * H * 128))):
                assert float((err[:, cols] / tol[:, cols]).max()) > 1.0, (S, H, family, name)
            assert float((err[:, 2 * H * 128:] / tol[:, 2 * H * 128:]).max()) <= 1.0          # dv does not pass the rotation
