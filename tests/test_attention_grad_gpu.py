"""The gradient-pass attention kernels -- csrc/causal_attention.hip (causal_fwd_kernel, causal_dq_kernel,
causal_dkv_kernel) and csrc/b1_attention.hip -- through `ops`, element by element against the float64 references and the
per-element error bounds of oracle/kernels.py (attention_ref, b1_attention_ref), at the smallest shapes that reach each
path: around the 16-row tile, the 32-row chunk and the 64-row workgroup, even and odd chunk counts (the two wave halves
unequal), prefixes on and off the chunk edges, every head width, grouped heads, every key visible, strided views, the
`into=` layout, the two-tiles-per-wave forward; on flat, sharp, ramped and per-key-scaled inputs (K.attention_inputs).
A whole-tensor maximum is set by the long rows; here a short row is held to its own size.  Every launch runs twice, bit
for bit.  tests/test_attention_refs.py shows on the CPU that a correct fp32 restatement of the kernels passes these
bounds and that a subtly wrong one does not.  Every test prints its worst error / bound ratio per output (pytest -s)."""

import functools

import pytest
import torch

from oracle import kernels as K
from oracle.kernels import AttnCase

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
NAMES = ("o", "lse2", "dq", "dk", "dv")


@functools.lru_cache(maxsize=None)
def _case(case, dt, family):
    """(q, k, v, d_out) on the device and their float64 reference, computed once for all tests."""
    q, k, v, do = (t.to(DEV) for t in K.attention_inputs(case, dt, family))
    return q, k, v, do, K.attention_ref(q, k, v, do, case.Dh ** -0.5, case.causal, dt)


def _launch(q, k, v, do, case, into=None):
    """Forward and backward through ops, each launch twice and compared bit for bit: {o, lse2, dq, dk, dv}."""
    from bimodalattack_amd import ops
    scale = case.Dh ** -0.5
    assert ops.causal_attention_ok(q, k, v)
    o, lse2 = ops.causal_attention(q, k, v, scale, case.causal)
    o2, lse2b = ops.causal_attention(q, k, v, scale, case.causal)
    assert torch.equal(o, o2) and torch.equal(lse2, lse2b), case
    dq, dk, dv = ops.causal_attention_bwd(q, k, v, o, lse2, do, scale, into=into, causal=case.causal)
    first = [t.clone() for t in (dq, dk, dv)]
    again = ops.causal_attention_bwd(q, k, v, o, lse2, do, scale, into=into, causal=case.causal)
    assert all(torch.equal(a, b) for a, b in zip(first, again)), case
    assert o.shape == q.shape and lse2.shape == (case.H, case.Lq) and dq.shape == q.shape and dk.shape == dv.shape == k.shape
    return {"o": o, "lse2": lse2, "dq": dq, "dk": dk, "dv": dv}


def _hold(got, ref, dt, label, worst):
    rs = K.attention_ratios(got, ref, dt)
    for name, (r, el) in rs.items():
        worst[name] = max(worst.get(name, 0.0), r)
    bad = {n: rs[n] for n in rs if not rs[n][0] <= 1.0}
    assert not bad, (label, bad)                                   # name -> (error / bound, element)


def _report(what, worst):
    print(f"{what}: worst error/bound " + " ".join(f"{n}={worst[n]:.3f}" for n in worst))


@pytest.mark.parametrize("family", K.ATTN_FAMILIES)
@pytest.mark.parametrize("dt", DTYPES)
def test_causal_attention_per_element_at_every_tile_edge(dt, family):
    """K.ATTN_SHAPES at 128-wide heads, two heads."""
    worst = {}
    for Lq, Lk in K.ATTN_SHAPES:
        case = AttnCase(Lq, Lk, 2, 2, 128, True)
        q, k, v, do, ref = _case(case, dt, family)
        _hold(_launch(q, k, v, do, case), ref, dt, (tuple(case), family), worst)
    _report(f"causal Dh=128 {dt} {family}", worst)


@pytest.mark.parametrize("family", K.ATTN_FAMILIES)
@pytest.mark.parametrize("dt", DTYPES)
def test_causal_attention_per_element_head_widths_groups_and_all_visible(dt, family):
    """The other cases of K.attention_cases(): 64-, 72- and 256-wide heads (72: 96-wide LDS images with zero columns, the
    outputs' last 8 dims a partly real tile; 256: two pieces per thread, the dk/dv launch splitting the output dims), four
    query heads over two and over one key/value head (the group's sum inside the launch), every key visible."""
    worst = {}
    for case in K.attention_cases()[len(K.ATTN_SHAPES):]:
        q, k, v, do, ref = _case(case, dt, family)
        _hold(_launch(q, k, v, do, case), ref, dt, (tuple(case), family), worst)
    _report(f"causal widths/groups/all-visible {dt} {family}", worst)


@pytest.mark.parametrize("dt", DTYPES)
def test_causal_attention_strided_views_of_one_fused_projection(dt):
    """q / k / v as views of one (Lk, (H + 2 Hkv) Dh + 8) buffer, the queries its last Lq rows: the same bits as from
    contiguous operands, and so within the same bounds."""
    worst = {}
    for case in (AttnCase(33, 33, 2, 2, 128, True), AttnCase(65, 65, 2, 2, 72, True), AttnCase(20, 84, 2, 2, 128, True),
                 AttnCase(65, 200, 4, 2, 128, True)):
        for family in ("randn", "sharp"):
            q, k, v, do, ref = _case(case, dt, family)
            Lq, Lk, H, Hkv, Dh, _ = case
            fused = torch.full((Lk, (H + 2 * Hkv) * Dh + 8), 3.0, device=DEV, dtype=dt)
            qs = fused[Lk - Lq:, :H * Dh].view(Lq, H, Dh)
            ks = fused[:, H * Dh:(H + Hkv) * Dh].view(Lk, Hkv, Dh)
            vs = fused[:, (H + Hkv) * Dh:(H + 2 * Hkv) * Dh].view(Lk, Hkv, Dh)
            qs.copy_(q), ks.copy_(k), vs.copy_(v)
            assert not qs.is_contiguous() and not ks.is_contiguous()
            got = _launch(qs, ks, vs, do, case)
            _hold(got, ref, dt, (tuple(case), family), worst)
            plain = _launch(q, k, v, do, case)
            assert all(torch.equal(got[n], plain[n]) for n in NAMES), (case, family)
    _report(f"causal strided views {dt}", worst)


@pytest.mark.parametrize("dt", DTYPES)
def test_causal_attention_bwd_into_a_fused_gradient_buffer(dt):
    """`into=` a (L, 3, H, Dh) buffer that sits inside a larger allocation: dq / dk / dv are the same bits as the fresh
    tensors', and the 64 elements in front of and behind the buffer stay as they were.  At 72-wide heads a lane's
    4-element store past the real width would land in the next head or the next of the three views."""
    from bimodalattack_amd import ops
    worst = {}
    for case in (AttnCase(1, 1, 2, 2, 128, True), AttnCase(33, 33, 2, 2, 128, True), AttnCase(65, 65, 2, 2, 128, True),
                 AttnCase(129, 129, 2, 2, 128, True), AttnCase(33, 33, 2, 2, 72, True), AttnCase(65, 65, 2, 2, 256, True)):
        q, k, v, do, ref = _case(case, dt, "randn")
        L, H, Dh = case.Lq, case.H, case.Dh
        n, guard = L * 3 * H * Dh, 64
        flat = torch.empty(n + 2 * guard, device=DEV, dtype=dt)
        flat.view(torch.int16).fill_(0x7b7b)
        before = flat.clone()
        into = flat[guard:guard + n].view(L, 3, H, Dh)
        got = _launch(q, k, v, do, case, into=into)
        assert got["dq"].data_ptr() == into.data_ptr() and got["dv"].data_ptr() == into[:, 2].data_ptr()
        assert torch.equal(flat[:guard].view(torch.int16), before[:guard].view(torch.int16)), case
        assert torch.equal(flat[guard + n:].view(torch.int16), before[guard + n:].view(torch.int16)), case
        _hold(got, ref, dt, tuple(case), worst)
        fresh = ops.causal_attention_bwd(q, k, v, got["o"], got["lse2"], do, Dh ** -0.5, causal=case.causal)
        assert all(torch.equal(a, b) for a, b in zip(fresh, (got["dq"], got["dk"], got["dv"]))), case
    _report(f"causal into= {dt}", worst)


@pytest.mark.parametrize("dt", DTYPES)
def test_causal_attention_two_tiles_per_wave_forward(dt):
    """The 72-wide forward with two query tiles per wave (128 rows per workgroup; by default from 1024 rows), reached at
    test size through the library's plan knob: one workgroup and a second of two rows, causal and not; the backward then
    runs from its output."""
    from bimodalattack_amd.native import lib
    worst = {}
    try:
        lib.bma_causal_attention_set_plan(1)
        for case in K.ATTN_TWO_TILE_CASES:
            for family in K.ATTN_FAMILIES:
                q, k, v, do, ref = _case(case, dt, family)
                _hold(_launch(q, k, v, do, case), ref, dt, (tuple(case), family), worst)
    finally:
        lib.bma_causal_attention_set_plan(1024)
    _report(f"causal two-tile forward {dt}", worst)


# ------------------------------------------------------------------ bma_b1_attention
@functools.lru_cache(maxsize=None)
def _b1_case(S, H, dt, family):
    qkv, cos, sin, do = K.b1_inputs(S, H, dt, family)
    big = torch.zeros((S, 3 * H * 128 + 64), device=DEV, dtype=dt)
    view = big[:, :3 * H * 128]                                    # a row stride wider than the row
    view.copy_(qkv)
    cos, sin, do = cos.to(DEV), sin.to(DEV), do.to(DEV)
    return view, cos, sin, do, K.b1_attention_ref(view, cos, sin, H, 128 ** -0.5, do, dt)


@pytest.mark.parametrize("family", K.ATTN_FAMILIES)
@pytest.mark.parametrize("dt", DTYPES)
def test_b1_attention_per_element(dt, family):
    """Rotary + attention + its backward in one launch each way, S on and off the 16-row tiles up to the 80-token limit,
    one head and three, qkv a view of wider rows: o, the natural-log lse and d(qkv) -- dq and dk through the inverse
    rotation -- against K.b1_attention_ref."""
    from bimodalattack_amd import ops
    worst = {}
    for S in K.B1_S:
        for H in K.B1_H:
            qkv, cos, sin, do, ref = _b1_case(S, H, dt, family)
            assert ops.b1_attention_ok(qkv, cos, H, H, 128) and qkv.stride(0) == 3 * H * 128 + 64
            scale = 128 ** -0.5
            o, lse = ops.b1_attention(qkv, cos, sin, H, scale)
            o2, lse_b = ops.b1_attention(qkv, cos, sin, H, scale)
            dqkv = ops.b1_attention_bwd(qkv, cos, sin, o, lse, do, H, scale)
            assert torch.equal(o, o2) and torch.equal(lse, lse_b) and torch.equal(dqkv, ops.b1_attention_bwd(qkv, cos, sin, o, lse, do, H, scale))
            assert o.shape == (S, H * 128) and lse.shape == (H, S) and dqkv.shape == (S, 3 * H * 128)
            rs = K.b1_attention_ratios({"o": o, "lse": lse, "dqkv": dqkv}, ref)
            for name, (r, el) in rs.items():
                worst[name] = max(worst.get(name, 0.0), r)
            bad = {n: rs[n] for n in rs if not rs[n][0] <= 1.0}
            assert not bad, (S, H, family, bad)                    # name -> (error / bound, (row, column) or (head, row))
    _report(f"b1 {dt} {family}", worst)
