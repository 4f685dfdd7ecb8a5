"""The backward elementwise kernels of csrc/fused_elementwise.hip -- rmsnorm_bwd_kernel, swiglu_bwd_kernel and the rotary
kernel with sin_sign = -1 -- through the `ops` autograd Functions, element by element against the float64 references
and error bounds of oracle/kernels.py, on every dispatch path: 1 to 4 chunks per lane with full and partly filled last
rounds, one chunk per row, the three dtypes, both activations and layouts, the grid-stride loop's second pass.
tests/test_backward_refs.py shows on the CPU that a correct fp32 evaluation passes these bounds and that a subtly wrong
one does not.  Every test prints its worst error / bound ratio (pytest -s)."""

import functools

import pytest
import torch

from oracle import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def _dev(*ts):
    return [t.to(DEV) for t in ts]


# ------------------------------------------------------------------ RMSNorm backward
def _norm_backward(x, w, dy, dsum, eps, gemma):
    from bimodalattack_amd import ops
    if dsum is None:
        xa = x.clone().requires_grad_()
        (dx,) = torch.autograd.grad(ops.RMSNormFn.apply(xa, w, eps, gemma), xa, dy)
        return dx
    # residual + 0 is the residual, bit for bit: the norm's input is x
    ra, ha = x.clone().requires_grad_(), torch.zeros_like(x).requires_grad_()
    s, y = ops.AddRMSNormFn.apply(ra, ha, w, eps, gemma)
    assert torch.equal(s.detach(), x)
    dr, dh = torch.autograd.grad([s, y], [ra, ha], [dsum, dy])
    assert torch.equal(dr, dh)
    return dr


@pytest.mark.parametrize("with_dsum", [False, True])
@pytest.mark.parametrize("gemma", [False, True])
@pytest.mark.parametrize("dt", DTYPES)
def test_rmsnorm_bwd_vs_float64(dt, gemma, with_dsum):
    """RMSNormFn (without dsum) and AddRMSNormFn with gradients on both outputs (with), at every row width of
    K.NORM_BWD_D and 1 and 6 rows (five of the six are edge rows: K.norm_bwd_inputs); each launch twice, bit for bit."""
    worst = 0.0
    for D in K.NORM_BWD_D[dt]:
        for rows in (1, 6):
            x, w, dy, dsum = _dev(*K.norm_bwd_inputs(rows, D, dt, gemma))
            ds = dsum if with_dsum else None
            eps = K.NORM_BWD_EPS[gemma]
            got = _norm_backward(x, w, dy, ds, eps, gemma)
            assert got.shape == x.shape and got.dtype == dt
            r = K.norm_bwd_ratio(got, x, w, dy, eps, gemma, ds, dt)
            worst = max(worst, r)
            assert r <= 1.0, (D, rows, r)
            assert torch.equal(_norm_backward(x, w, dy, ds, eps, gemma), got), (D, rows)
    print(f"rmsnorm_bwd {dt} gemma={gemma} dsum={with_dsum}: worst error/bound {worst:.3f}")


@pytest.mark.parametrize("dt", DTYPES)
def test_rmsnorm_bwd_refuses_wide_rows_and_skips_empty_ones(dt):
    """A row beyond 16 KiB is refused by the forward (through ops) and by the backward's C entry point (BMA_ELIMIT)
    before anything is launched; rows == 0 returns at once and leaves the output alone."""
    from bimodalattack_amd import ops
    from bimodalattack_amd.native import BmaError, lib
    es = torch.empty((), dtype=dt).element_size()
    ne = 16 // es
    D = 16384 // es + ne                                   # one chunk past the limit
    x = torch.randn((2, D), device=DEV).to(dt)
    w = torch.ones(D, device=DEV, dtype=dt)
    dx = torch.full_like(x, 7.0)
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(BmaError, match="size beyond kernel limit"):
        ops.RMSNormFn.apply(x.clone().requires_grad_(), w, 1e-5, False)
    with pytest.raises(BmaError, match="size beyond kernel limit"):
        ops.AddRMSNormFn.apply(x.clone().requires_grad_(), x.clone().requires_grad_(), w, 1e-5, True)
    for gemma in (0, 1):
        assert lib.bma_rmsnorm_bwd(x.data_ptr(), w.data_ptr(), x.data_ptr(), 1e-5, 2, D, ops._dt(x), gemma, dx.data_ptr(), st) == -5
        assert lib.bma_add_rmsnorm_bwd(x.data_ptr(), w.data_ptr(), x.data_ptr(), x.data_ptr(), 1e-5, 2, D, ops._dt(x), gemma,
                                       dx.data_ptr(), st) == -5
    D = 16384 // es                                        # the widest row there is, no rows
    assert lib.bma_rmsnorm_bwd(x.data_ptr(), w.data_ptr(), x.data_ptr(), 1e-5, 0, D, ops._dt(x), 0, dx.data_ptr(), st) == 0
    assert lib.bma_add_rmsnorm_bwd(x.data_ptr(), w.data_ptr(), x.data_ptr(), x.data_ptr(), 1e-5, 0, D, ops._dt(x), 1,
                                   dx.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all())
    xe = torch.zeros((0, D), device=DEV, dtype=dt).requires_grad_()
    (ge,) = torch.autograd.grad(ops.RMSNormFn.apply(xe, w[:D], 1e-5, True), xe, torch.zeros((0, D), device=DEV, dtype=dt))
    assert ge.shape == (0, D)


# ------------------------------------------------------------------ gated activation backward
def _interleave(g, u):
    ne = 16 // g.element_size()
    return torch.stack([g.view(-1, ne), u.view(-1, ne)], 1).reshape(-1).contiguous()


def _gated_backward(gate, up, dy, act, il):
    """(d_gate, d_up) from SwiGLUFn, or from SwiGLUInterleavedFn on the chunk-interleaved array, de-interleaved."""
    from bimodalattack_amd import ops
    if not il:
        a, b = gate.clone().requires_grad_(), up.clone().requires_grad_()
        return torch.autograd.grad(ops.SwiGLUFn.apply(a, b, act), (a, b), dy)
    ne = 16 // gate.element_size()
    gu = _interleave(gate, up).requires_grad_()
    (d,) = torch.autograd.grad(ops.SwiGLUInterleavedFn.apply(gu, act), gu, dy)
    d = d.view(-1, 2, ne)
    return d[:, 0].reshape(-1), d[:, 1].reshape(-1)


@pytest.mark.parametrize("il", [False, True])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dt", DTYPES)
def test_gated_act_bwd_vs_float64(dt, act, il):
    """SwiGLUFn / SwiGLUInterleavedFn, SiLU (0) and GELU-tanh (1), n = 8, 24 and 65,536 of K.gated_bwd_inputs: d_gate
    within its bound, d_up inside the interval its dtype-rounded activation allows; the interleaved form against the
    same reference, not against the two-array kernel.  Each launch twice, bit for bit."""
    for n in K.GATED_BWD_N:
        gate, up, dy = _dev(*K.gated_bwd_inputs(n, dt))
        dg, du = _gated_backward(gate, up, dy, act, il)
        assert dg.dtype == dt and du.dtype == dt and dg.shape == (n,) and du.shape == (n,)
        rg, ru, share = K.gated_bwd_ratios(dg, du, gate, up, dy, act, dt)
        print(f"gated_act_bwd {dt} act={act} il={il} n={n}: d_gate error/bound {rg:.3f}, d_up {ru:.3f}, ambiguous {share:.4f}")
        assert rg <= 1.0 and ru <= 1.0, (n, rg, ru)
        if n == 65536 and dt != torch.float32:
            assert share <= (0.01 if act == 0 else 0.25), share
        again = _gated_backward(gate, up, dy, act, il)
        assert torch.equal(again[0], dg) and torch.equal(again[1], du), n


@functools.lru_cache(maxsize=1)
def _wrap_inputs():
    return K.gated_bwd_inputs(K.GATED_BWD_WRAP_N, torch.bfloat16)


@pytest.mark.parametrize("il", [False, True])
def test_gated_act_bwd_second_pass_of_the_grid_stride_loop(il):
    """1,048,576 + 256 + 3 chunks in bf16: swiglu_bwd_kernel's grid is capped at 4096 x 256 lanes, so its loop makes a
    second, partial pass -- the same bounds, with the float64 reference on the device.  The outputs' memory is poisoned
    first, so that chunks a pass skipped cannot hold a right answer.  The forward (bma_gated_act, bma_gated_act_il) has no
    such loop and no cap -- one slab of 1024 chunks per workgroup, as many workgroups as it takes -- so it runs at this
    size too, against fn(a)*b as test_swiglu_vs_eager compares it."""
    from bimodalattack_amd import ops
    dt = torch.bfloat16
    gate, up, dy = _dev(*_wrap_inputs())
    n = gate.numel()
    assert n == 8390680 and n * 2 // 16 > 4096 * 256
    for act, fn in ((0, torch.nn.functional.silu), (1, lambda t: torch.nn.functional.gelu(t, approximate="tanh"))):
        poison = [torch.full((2 * n if il else n,), float("nan"), device=DEV, dtype=dt) for _ in range(1 if il else 2)]
        del poison
        dg, du = _gated_backward(gate, up, dy, act, il)
        rg, ru, share = K.gated_bwd_ratios(dg, du, gate, up, dy, act, dt)
        print(f"gated_act_bwd wrap act={act} il={il}: d_gate error/bound {rg:.3f}, d_up {ru:.3f}, ambiguous {share:.4f}")
        assert rg <= 1.0 and ru <= 1.0, (act, rg, ru)
        assert share <= (0.01 if act == 0 else 0.25), share
        again = _gated_backward(gate, up, dy, act, il)
        assert torch.equal(again[0], dg) and torch.equal(again[1], du)
        want = fn(gate) * up
        got = ops.swiglu_il(_interleave(gate, up), act) if il else ops.swiglu(gate, up, act)
        if act == 0:
            assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        else:                                           # aten's partial last block is 1 fp32 ulp off its own main loop
            torch.testing.assert_close(got.float(), want.float(), rtol=2 * 2.0 ** -8, atol=0)


# ------------------------------------------------------------------ rotary backward
@pytest.mark.parametrize("dt", DTYPES)
def test_rope_bwd_is_rope_ref_bit_for_bit(dt):
    """RoPEFn's backward and ops.rope(inverse=True) against rope_ref(sign=-1): Dh 64, 128, 256; L 1, 65; two heads over
    a strided view of a fused projection; cos/sin shared by the batch or one per sample (B = 3).  The forward against
    rope_ref(sign=+1), and inverse(forward(x)) against x within K.rope_round_trip_tol."""
    from bimodalattack_amd import ops
    B, H = 3, 2
    worst = 0.0
    for Dh in (64, 128, 256):
        for L in (1, 65):
            for cb in (1, B):
                q, cos, sin, dq = K.rope_inputs(B, H, L, Dh, cb, dt)
                want_f, want_b = K.rope_ref(q, cos, sin, 1, dt), K.rope_ref(dq, cos, sin, -1, dt)
                # the views again on the device, over their whole projections
                qkv = q._base.to(DEV).requires_grad_()
                dqkv = dq._base.to(DEV)
                view = lambda t: t[..., H * Dh:2 * H * Dh].view(B, L, H, Dh).transpose(1, 2)
                cos, sin = _dev(cos, sin)
                y = ops.RoPEFn.apply(view(qkv), cos, sin)
                assert torch.equal(y.detach().double().cpu(), want_f), (Dh, L, cb)
                dqc = view(dqkv).contiguous()
                (g,) = torch.autograd.grad(y, qkv, dqc, retain_graph=True)
                assert torch.equal(view(g).double().cpu(), want_b), (Dh, L, cb)
                outside = g.clone()
                view(outside).zero_()
                assert not bool(outside.any())                                 # nothing flows to k and v
                inv = ops.rope(view(dqkv), cos, sin, inverse=True)            # the strided view itself
                assert torch.equal(inv.double().cpu(), want_b), (Dh, L, cb)
                (g2,) = torch.autograd.grad(y, qkv, dqc)
                assert torch.equal(g2, g) and torch.equal(ops.rope(view(dqkv), cos, sin, inverse=True), inv)
                back = ops.rope(y.detach(), cos, sin, inverse=True).double().cpu()
                r = ((back - q.double()).abs() / K.rope_round_trip_tol(q, dt)).max().item()
                worst = max(worst, r)
                assert r <= 1.0, (Dh, L, cb, r)
    print(f"rope {dt}: inverse(forward(x)) worst error/bound {worst:.3f}")
