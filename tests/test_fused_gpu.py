"""Fused RMSNorm / SwiGLU / RoPE kernels against the eager HuggingFace modules they
replace (GPU).  SwiGLU and RoPE keep every rounding point of the eager chain: bit-exact.
RMSNorm's mean is summed in a different order: <= 2 ulp of the model dtype on < 0.2 % of
elements (fp32: 2e-6 rel)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def ulp_diff(a, b):
    """Distance in representable values of a 16-bit float tensor."""
    ia = a.view(torch.int16).to(torch.int32)
    ib = b.view(torch.int16).to(torch.int32)
    ia = torch.where(ia < 0, -32768 - ia, ia)
    ib = torch.where(ib < 0, -32768 - ib, ib)
    return (ia - ib).abs()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("rows,D", [(22528, 4096), (37, 2560), (5, 32), (3, 8192), (64, 256),
                                    # short rows: several rows per workgroup, ragged last workgroup
                                    (1001, 256), (77, 128), (33, 64), (9, 8), (13, 512), (7, 40), (129, 200)])
def test_rmsnorm_vs_hf(dtype, rows, D):
    from bimodalattack_amd import ops
    from transformers.models.gemma3.modeling_gemma3 import Gemma3RMSNorm
    from transformers.models.llama.modeling_llama import LlamaRMSNorm
    g = torch.Generator(device=DEV).manual_seed(D)
    x = (torch.randn((rows, D), generator=g, device=DEV) * 3).to(dtype)
    if D * x.element_size() > 16384:                      # beyond the kernel's row limit: refused, not wrong
        from bimodalattack_amd.native import BmaError
        with pytest.raises(BmaError, match="size beyond kernel limit"):
            ops.rmsnorm(x, torch.ones(D, device=DEV, dtype=dtype), 1e-5)
        return
    for gemma, cls in ((False, LlamaRMSNorm), (True, Gemma3RMSNorm)):
        m = cls(D, eps=1e-5).to(DEV, dtype)
        with torch.no_grad():
            m.weight.copy_((torch.randn(D, generator=g, device=DEV) * 0.3 + (0.0 if gemma else 1.0)).to(dtype))
            want = m(x)
            got = ops.rmsnorm(x, m.weight, 1e-5, gemma)
        if dtype == torch.float32:
            np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=2e-6, atol=1e-7)
        else:
            d = ulp_diff(got, want)
            # a 1-ulp difference of the normalised value can become 2 ulp after the weight product
            stats = (int(d.max()), float((d > 0).float().mean()), float((d > 1).float().mean()))
            assert stats[0] <= 2 and stats[1] < 2e-3 and stats[2] < 1e-4, stats


def test_head_norm_on_transposed_view_is_copy_free():
    """Gemma's q_norm/k_norm see a (B,H,L,Dh) view of a (B,L,H,Dh) projection: the patched norm
    works in the memory order it finds and hands back the same kind of view."""
    from bimodalattack_amd.fused import FusedInference
    from transformers.models.gemma3.modeling_gemma3 import Gemma3RMSNorm

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.q_norm = Gemma3RMSNorm(256, eps=1e-6)

    h = Holder().to(DEV, torch.bfloat16)
    with torch.no_grad():
        h.q_norm.weight.copy_(torch.randn(256, device=DEV) * 0.2)
    base = torch.randn(3, 11, 8, 256, device=DEV).to(torch.bfloat16)
    x = base.transpose(1, 2)
    with torch.no_grad():
        want = h.q_norm(x)
        with FusedInference(h, True):
            got = h.q_norm(x)
    assert got.shape == want.shape and got.stride() == x.stride()          # still the transposed view
    d = ulp_diff(got.contiguous(), want.contiguous())
    assert int(d.max()) <= 2 and float((d > 0).float().mean()) < 2e-3
    xg = x.clone().requires_grad_()
    with FusedInference(h, True):
        y = h.q_norm(xg)
    ge, = torch.autograd.grad(h.q_norm(xg), xg, torch.ones_like(want))
    gf, = torch.autograd.grad(y, xg, torch.ones_like(y))
    np.testing.assert_allclose(gf.float().cpu().numpy(), ge.float().cpu().numpy(), rtol=5e-2, atol=5e-2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_swiglu_vs_eager(dtype):
    from bimodalattack_amd import ops
    g = torch.Generator(device=DEV).manual_seed(3)
    for shape in [(512, 44, 11008), (3, 5, 64), (1, 1, 8)]:
        a = (torch.randn(shape, generator=g, device=DEV) * 4).to(dtype)
        b = (torch.randn(shape, generator=g, device=DEV) * 2).to(dtype)
        for act, fn in ((ops.ACT_SILU, torch.nn.functional.silu),
                        (ops.ACT_GELU_TANH, lambda t: torch.nn.functional.gelu(t, approximate="tanh"))):
            want = fn(a) * b
            got = ops.swiglu(a, b, act)
            if dtype == torch.float32:
                np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=3e-6, atol=1e-30)
            elif act == ops.ACT_SILU or a.numel() % 4096 == 0:
                assert torch.equal(got.view(torch.int16), want.view(torch.int16)), act
            else:
                # aten's gelu is not self-consistent: the partial last block of its launch runs a
                # separately compiled loop where 0.5x(1+t) became fma(0.5x, t, 0.5x) -- 1 fp32 ulp
                # away, and +0 instead of -0 once tanh saturates.  The kernel follows the main loop.
                ulp = 2.0 ** (-8 if dtype == torch.bfloat16 else -11)
                np.testing.assert_allclose(got.float().cpu().numpy(), want.float().cpu().numpy(), rtol=2 * ulp, atol=0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_interleaved_gate_up_equals_separate(dtype):
    """gate_proj / up_proj as one product against chunk-interleaved weights + the interleaved gate kernel:
    the weight layout puts gate and up rows in alternating 16-byte chunks, the kernel output is bit-identical
    to the two-array kernel on the de-interleaved halves, forward and backward; the whole MLP agrees with the
    HuggingFace module to GEMM rounding."""
    from bimodalattack_amd import ops
    g = torch.Generator(device=DEV).manual_seed(11)
    I, D, M = 11008, 512, 77
    wg = (torch.randn((I, D), generator=g, device=DEV) * 0.05).to(dtype)
    wu = (torch.randn((I, D), generator=g, device=DEV) * 0.05).to(dtype)
    w = ops.interleave_gate_up(wg, wu)
    assert w.shape == (2 * I, D)
    assert torch.equal(w[:8], wg[:8]) and torch.equal(w[8:16], wu[:8]) and torch.equal(w[16:24], wg[8:16])
    x = torch.randn((M, D), generator=g, device=DEV).to(dtype)
    y = torch.nn.functional.linear(x, w)                                   # (M, 2I) interleaved
    yg = y.view(M, I // 8, 2, 8)[:, :, 0].reshape(M, I).contiguous()
    yu = y.view(M, I // 8, 2, 8)[:, :, 1].reshape(M, I).contiguous()
    for act in (ops.ACT_SILU, ops.ACT_GELU_TANH):
        assert torch.equal(ops.swiglu_il(y, act), ops.swiglu(yg, yu, act))
        yy = y.clone().requires_grad_()
        a, b = yg.clone().requires_grad_(), yu.clone().requires_grad_()
        dy = torch.randn((M, I), generator=g, device=DEV).to(dtype)
        (d_il,) = torch.autograd.grad(ops.SwiGLUInterleavedFn.apply(yy, act), yy, dy)
        da, db = torch.autograd.grad(ops.SwiGLUFn.apply(a, b, act), (a, b), dy)
        assert torch.equal(d_il.view(M, I // 8, 2, 8)[:, :, 0].reshape(M, I), da)
        assert torch.equal(d_il.view(M, I // 8, 2, 8)[:, :, 1].reshape(M, I), db)
    # a ragged tail (fewer chunks than one workgroup slab) and 3-D inputs
    z = torch.randn((3, 5, 48), generator=g, device=DEV).to(dtype)
    zg = z.view(3, 5, 3, 2, 8)[..., 0, :].reshape(3, 5, 24).contiguous()
    zu = z.view(3, 5, 3, 2, 8)[..., 1, :].reshape(3, 5, 24).contiguous()
    assert torch.equal(ops.swiglu_il(z), ops.swiglu(zg, zu))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_rope_vs_hf(dtype):
    from bimodalattack_amd import ops
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb
    g = torch.Generator(device=DEV).manual_seed(5)
    for B, L, H, Hk, Dh in [(64, 44, 32, 32, 128), (3, 7, 8, 2, 256), (2, 5, 4, 4, 16)]:
        q = torch.randn((B, L, H * Dh), generator=g, device=DEV).to(dtype).view(B, L, H, Dh).transpose(1, 2)
        k = torch.randn((B, L, Hk * Dh), generator=g, device=DEV).to(dtype).view(B, L, Hk, Dh).transpose(1, 2)
        ang = torch.rand((1, L, Dh // 2), generator=g, device=DEV) * 6.28
        emb = torch.cat([ang, ang], dim=-1)
        cos, sin = emb.cos().to(dtype), emb.sin().to(dtype)
        wq, wk = apply_rotary_pos_emb(q, k, cos, sin)
        gq, gk = ops.rope_(q.clone(), cos, sin), ops.rope_(k.clone(), cos, sin)
        if dtype == torch.float32:
            np.testing.assert_allclose(gq.cpu().numpy(), wq.cpu().numpy(), rtol=1e-6, atol=1e-7)
            np.testing.assert_allclose(gk.cpu().numpy(), wk.cpu().numpy(), rtol=1e-6, atol=1e-7)
        else:
            assert torch.equal(gq.contiguous().view(torch.int16), wq.contiguous().view(torch.int16))
            assert torch.equal(gk.contiguous().view(torch.int16), wk.contiguous().view(torch.int16))
        # per-batch cos/sin
        cosb, sinb = cos.expand(B, -1, -1).contiguous(), sin.expand(B, -1, -1).contiguous()
        assert torch.equal(ops.rope_(q.clone(), cosb, sinb), gq)
        # out of place (what the gradient pass uses): same bits; the inverse flag equals rotating with -sin
        assert torch.equal(ops.rope(q, cos, sin), gq) and torch.equal(ops.rope(k, cos, sin), gk)
        assert torch.equal(ops.rope(q, cos, sin, inverse=True), ops.rope_(q.clone(), cos, -sin))


def _small_llama(dtype):
    """head_dim 32 so the rotary kernel qualifies in 16-bit dtypes too."""
    from transformers import LlamaConfig, LlamaForCausalLM
    from bimodalattack_amd import synthetic as S
    cfg = LlamaConfig(vocab_size=264, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=256)
    cfg._attn_implementation = "sdpa"
    return S._build(LlamaForCausalLM, cfg, dtype, DEV, 0, 0.2)


@pytest.mark.parametrize("kind,dtype", [("llama", torch.bfloat16), ("llama", torch.float16), ("llava", torch.float32),
                                        ("gemma3", torch.float32), ("gemma3", torch.bfloat16)])
def test_fused_context_patches_and_restores(kind, dtype):
    """Inside the context the model's logits move by no more than rounding; the kernels are
    really called; outside, the model is untouched."""
    from bimodalattack_amd import native, synthetic as S
    from bimodalattack_amd.fused import FusedInference
    model = _small_llama(dtype) if kind == "llama" else S.tiny_case(kind, dtype=dtype, device=DEV)[0]
    D = model.get_input_embeddings().weight.shape[1]
    x = (torch.randn((6, 12, D), device=DEV) * 0.5).to(dtype)
    fused = FusedInference(model)
    assert fused.norms and fused.rope_modules and fused.mlps
    with torch.no_grad():
        want = model(inputs_embeds=x, use_cache=False).logits.float()
        native.profile_enable(True)
        with fused:
            got = model(inputs_embeds=x, use_cache=False).logits.float()
        prof = native.profile_read()
        native.profile_enable(False)
        again = model(inputs_embeds=x, use_cache=False).logits.float()
    assert prof["rmsnorm"]["launches"] > 0
    # tiny test models have head_dim 8: too short for 16-byte chunks in 16-bit dtypes
    assert (prof["rope"]["launches"] > 0) == (kind == "llama" or dtype == torch.float32)
    assert prof["swiglu"]["launches"] > 0 and fused.mlps            # SiLU (llama) and GELU-tanh (gemma) gates
    assert torch.equal(again, want)                                     # restored
    assert not any("forward" in m.__dict__ for m in model.modules())
    tol = 1e-4 if dtype == torch.float32 else 6e-2
    assert float((got - want).abs().max()) <= tol * max(1.0, float(want.abs().max()))
    # with autograd on, the fused Functions record a graph: input gradients equal eager autograd's
    xe = x.clone().requires_grad_()
    ge, = torch.autograd.grad(model(inputs_embeds=xe, use_cache=False).logits.float().square().mean(), xe)
    xf = x.clone().requires_grad_()
    with fused:
        y = model(inputs_embeds=xf, use_cache=False).logits
        assert y.requires_grad
        gf, = torch.autograd.grad(y.float().square().mean(), xf)
    if kind == "llama" and dtype != torch.float32:
        # 72 rows: the transposed-weight backward ran -- q/k/v as one fused projection per layer, gate/up as one
        # (chunk-interleaved) projection, o and down each
        kinds = [k[0] for k in fused._copies.d]
        assert len(fused.qkv) == 2 and len(fused.linears) == 2 * 7 and \
            {k: kinds.count(k) for k in set(kinds)} == {"wqkv": 2, "wqkv_t": 2, "wgu": 2, "wgu_t": 2, "wt": 4}
        # the copies belong to the model: a second context object on it finds them, and a changed weight drops its copy
        again = FusedInference(model)
        assert again._copies is fused._copies
        lin = fused.linears[0]
        key = next(k for k in fused._copies.d if k[0] == "wt")
        owner = next(m for m in fused.linears if id(m) == key[1])
        old = fused._copies.get(key, (owner.weight,))
        with torch.no_grad():
            owner.weight.mul_(1.0)                      # an in-place write bumps the version counter
        assert old is not None and fused._copies.get(key, (owner.weight,)) is None
    gtol = 1e-4 if dtype == torch.float32 else 8e-2
    assert float((gf.float() - ge.float()).abs().max()) <= gtol * float(ge.float().abs().max())
    assert not any("forward" in m.__dict__ for m in model.modules())


def test_products_just_above_whole_tile_rounds_run_as_two_calls():
    """fused.round_cut / ROUND_SPLIT: inside the fused context a no-grad o_proj / down_proj product whose row count sits just above a
    whole number of 256 x 256 tile rounds (4352 rows x 4096 columns on this chip's CUs: 17 x 16 = 272 tiles) is issued as two library
    calls into row slices of ONE output -- the same rows, so the same numbers up to the rounding of whichever solution serves each
    call (fp32 accumulation, one rounding to bf16) -- and a product that does not qualify, a recording autograd, or the switch turned
    off leave the module's own forward in charge."""
    from bimodalattack_amd import fused as F_
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count

    class Block(torch.nn.Module):               # what FusedInference looks for: a block with bias-free projections
        def __init__(self):
            super().__init__()
            self.q_proj = torch.nn.Linear(512, 64, bias=False)
            self.o_proj = torch.nn.Linear(512, 4096, bias=False)
            self.layer_idx = 0

    g = torch.Generator(device=DEV).manual_seed(2)
    blk = Block().to(DEV, torch.bfloat16)
    with torch.no_grad():
        blk.o_proj.weight.copy_(torch.randn((4096, 512), generator=g, device=DEV) * 0.05)
    rows = 256 * (cus // 16 + 1)                # one row tile behind the first round boundary (4352 on 256 CUs)
    assert F_.round_cut(rows, 4096, cus) == rows - 256
    x = torch.randn((1, rows, 512), generator=g, device=DEV).to(torch.bfloat16)
    want = torch.nn.functional.linear(x.double(), blk.o_proj.weight.detach().double())
    calls = []
    real_mm = torch.mm

    def counting_mm(a, b, out=None):
        calls.append(tuple(a.shape))
        return real_mm(a, b, out=out)

    fi = F_.FusedInference(blk, True)
    try:
        torch.mm = counting_mm
        with torch.no_grad(), fi:
            got = blk.o_proj(x)
            assert calls == [(rows - 256, 512), (256, 512)], calls
            calls.clear()
            small = blk.o_proj(x[:, :rows - 256])               # whole rounds exactly: one call, the module's own
            assert calls == [] and small.shape == (1, rows - 256, 4096)
        with fi:
            xg = x.clone().requires_grad_()
            y = blk.o_proj(xg)                                  # autograd records: never split
            assert calls == [] and y.requires_grad
        old = F_.ROUND_SPLIT
        F_.ROUND_SPLIT = False
        try:
            with torch.no_grad(), fi:
                off = blk.o_proj(x)
            assert calls == []
        finally:
            F_.ROUND_SPLIT = old
    finally:
        torch.mm = real_mm
    assert got.shape == (1, rows, 4096) and got.dtype == torch.bfloat16
    for t in (got, off):
        err = (t.double() - want).abs() / want.abs().clamp_min(1.0)
        assert float(err.max()) <= 2.0 ** -8, float(err.max())      # one bf16 rounding of an fp32-accumulated sum


# ------------------------------------------------------------------ shared-prefix attention
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_attn_merge_and_shared_prefix_equal_full_attention(dtype):
    """Two partial attentions + merge == attention over [prefix | own tokens] with a causal
    mask on the own part, to the dtype's rounding."""
    from bimodalattack_amd import prefix_attention as pa
    g = torch.Generator(device=DEV).manual_seed(11)
    for B, H, Hkv, L, P, Dh in [(16, 8, 8, 44, 21, 128), (3, 4, 2, 7, 50, 64), (1, 2, 2, 5, 1, 32)]:
        q = torch.randn((B, L, H, Dh), generator=g, device=DEV).to(dtype).transpose(1, 2)
        k = torch.randn((B, L, Hkv, Dh), generator=g, device=DEV).to(dtype).transpose(1, 2)
        v = torch.randn((B, L, Hkv, Dh), generator=g, device=DEV).to(dtype).transpose(1, 2)
        kp = torch.randn((1, Hkv, P, Dh), generator=g, device=DEV).to(dtype)
        vp = torch.randn((1, Hkv, P, Dh), generator=g, device=DEV).to(dtype)

        class Layer:
            keys, values = kp, vp

        kv = pa.SharedPrefixKV(type("C", (), {"layers": [Layer]})())
        mod = type("M", (), {"layer_idx": 0})()
        pa._ACTIVE.append(kv)
        try:
            out, _ = pa.shared_prefix_attention(mod, q, k, v, None, scaling=Dh ** -0.5)
        finally:
            pa._ACTIVE.pop()
        rep = H // Hkv
        fk = torch.cat([kp.expand(B, -1, -1, -1), k], 2).repeat_interleave(rep, 1).float()
        fv = torch.cat([vp.expand(B, -1, -1, -1), v], 2).repeat_interleave(rep, 1).float()
        mask = torch.ones(L, P + L, dtype=torch.bool, device=DEV)
        mask[:, P:] = torch.tril(torch.ones(L, L, dtype=torch.bool, device=DEV))
        ref = torch.nn.functional.scaled_dot_product_attention(q.float(), fk, fv, attn_mask=mask, scale=Dh ** -0.5)
        tol = 2e-5 if dtype == torch.float32 else (2e-2 if dtype == torch.bfloat16 else 3e-3)
        assert out.shape == (B, L, H, Dh)
        assert float((out.float() - ref.transpose(1, 2)).abs().max()) < tol


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_shared_prefix_forward_equals_cache_forward(dtype):
    """Whole-model check on a small Llama: logits through the shared-prefix attention equal
    logits through the stock HF cache path."""
    from bimodalattack_amd.hf_adapter import HFAdapter
    from bimodalattack_amd import synthetic as S
    model = _small_llama(dtype)
    ad = HFAdapter(model, S.SyntheticProcessor(None), None)
    assert ad.shared_prefix_configs()
    D = model.get_input_embeddings().weight.shape[1]
    B, P, L, T = 6, 9, 12, 4
    g = torch.Generator(device=DEV).manual_seed(2)
    prefix = (torch.randn((1, P, D), generator=g, device=DEV) * 0.5).to(dtype)
    tail = (torch.randn((B, L, D), generator=g, device=DEV) * 0.5).to(dtype)
    with torch.no_grad():
        cache = ad.build_prefix(prefix)
        want = ad.target_logits(tail, T, cache=ad.expand_prefix(cache, B)).float()
        got = ad.target_logits_shared_prefix(tail, T, cache).float()
        again = ad.target_logits(tail, T, cache=ad.expand_prefix(cache, B)).float()
    assert torch.equal(again, want)                                   # attention implementation restored
    tol = 1e-4 if dtype == torch.float32 else 5e-2
    assert float((got - want).abs().max()) <= tol * max(1.0, float(want.abs().max()))


def test_gather_rows_and_mapped_merge_vs_torch():
    from bimodalattack_amd import ops
    g = torch.Generator(device=DEV).manual_seed(4)
    for dtype in (torch.bfloat16, torch.float32):
        src = torch.randn((37, 4, 64), generator=g, device=DEV).to(dtype)
        idx = torch.randint(0, 37, (101,), generator=g, device=DEV).to(torch.int32)
        assert torch.equal(ops.gather_rows(src, idx), src[idx.long()])
        # out-of-range indices are clamped, never read outside the source
        bad = torch.tensor([-5, 36, 37, 1000], device=DEV, dtype=torch.int32)
        assert torch.equal(ops.gather_rows(src, bad), src[torch.tensor([0, 36, 36, 36], device=DEV)])
        N, B2, L, H, Dh = 50, 5, 12, 4, 64
        o1 = torch.randn((N, H, Dh), generator=g, device=DEV).to(dtype)
        o2 = torch.randn((B2, L, H, Dh), generator=g, device=DEV).to(dtype)
        l1 = torch.randn((H, N), generator=g, device=DEV)
        l2 = torch.randn((B2, H, L), generator=g, device=DEV)
        rmap = torch.randperm(B2 * L, generator=g, device=DEV)[:N].to(torch.int32)
        got = ops.attn_merge_rows(o1, o2, l1, l2, rmap)
        # the padded-layout kernel on the rows picked out by hand is the reference
        o2r = o2.view(B2 * L, H, Dh)[rmap.long()]
        l2r = l2.permute(0, 2, 1).reshape(B2 * L, H)[rmap.long()]                     # (N,H)
        want = ops.attn_merge(o1.view(1, N, H, Dh), o2r.view(1, N, H, Dh).contiguous(), l1.contiguous(),
                              l2r.t().reshape(1, H, N).contiguous())
        assert torch.equal(got, want.view(N, H, Dh))


def _ragged_attention_reference(q, k, v, pk, pv, plan, P, scale):
    """fp32 loops over (candidate, query, head): softmax over [prefix | parent rows < first | own rows <= query]."""
    N, H, Dh = q.shape
    rep = H // k.shape[1]
    out = torch.zeros_like(q)
    for st, p0, ln in zip(plan["cstart"].tolist(), plan["cfirst"].tolist(), plan["clen"].tolist()):
        rows = list(range(p0)) + list(range(st, st + ln))
        K, V = k[rows], v[rows]
        if P:
            K, V = torch.cat([pk, K]), torch.cat([pv, V])
        for qi in range(ln):
            vis = P + p0 + qi + 1
            for h in range(H):
                w = torch.softmax((K[:vis, h // rep] @ q[st + qi, h]) * scale, 0)
                out[st + qi, h] = w @ V[:vis, h // rep]
    return out


def _row_scale_err(got, want64, floor=1e-2):
    """The worst (row, head) error in units of that row's OWN scale: max_d |got - want| / max(max_d |want|, floor).  `want64` is
    float64 attention on the same 16-bit operands; a flash kernel that rounds P to the 16-bit type before the P.V product and
    its output once stays within ~3 roundings (2^-8 each in bf16) of it -- the bound test_causal_attention_forward_and_backward_
    match_float64 holds the batch-1 kernels to (an absolute 2e-2 on outputs of 0.1-1 was ~5x looser)."""
    d = (got.double() - want64).abs().amax(-1)
    return float((d / want64.abs().amax(-1).clamp_min(floor)).max())


def _ragged_candidate_reference64(q, k, v, pk, pv, st, p0, ln, P, scale):
    """float64 attention of ONE candidate of a ragged row list on the device, every head: queries q[st:st+ln] over
    [prefix | parent rows < p0 | own rows <= query] (the loop of _ragged_attention_reference, vectorised).  (ln, H, Dh)."""
    H, Hk = q.shape[1], k.shape[1]
    rep = H // Hk
    rows = torch.cat([torch.arange(p0, device=q.device), torch.arange(st, st + ln, device=q.device)])
    K = torch.cat([pk, k[rows]]).double().repeat_interleave(rep, dim=1)          # (P + p0 + ln, H, Dh)
    V = torch.cat([pv, v[rows]]).double().repeat_interleave(rep, dim=1)
    s_ = torch.einsum("qhd,khd->hqk", q[st:st + ln].double(), K) * scale
    vis = (torch.arange(K.shape[0], device=q.device)[None, :] <= (P + p0 + torch.arange(ln, device=q.device))[:, None])
    w = torch.softmax(s_.masked_fill(~vis[None], float("-inf")), -1)
    return torch.einsum("hqk,khd->qhd", w, V)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("m,n_opt,L,T,P,H,Hk,Dh,merge", [
    (7, 5, 13, 4, 9, 4, 2, 32, False),        # grouped heads, one query tile
    (5, 6, 20, 5, 21, 8, 8, 128, False),      # two tiles, prefix not a multiple of the key chunk
    (5, 6, 44, 20, 40, 4, 4, 64, False),      # three tiles (the C3 lengths)
    (3, 4, 50, 10, 0, 4, 2, 128, False),      # no prefix, four tiles
    (5, 6, 20, 5, 70, 8, 4, 128, True),       # prefix partial computed elsewhere, merged in the epilogue
    (3, 4, 303, 20, 20, 8, 4, 256, False),    # Gemma-3 joint block: 256-wide grouped heads, five 64-query stretches, streamed keys
    (4, 6, 100, 10, 21, 4, 4, 128, False),    # 121 keys x 128: past the resident-LDS budget, streamed, two stretches
    (5, 6, 70, 10, 5, 4, 2, 64, False),       # two stretches with every chunk resident in LDS
    (2, 3, 303, 5, 0, 2, 1, 256, True),       # long blocks + merged prefix partial
    # the long-block kernel (max_len >= 96 at 128 / 256-wide heads): head pairs per workgroup or single heads, two
    # 128-query stretches, four query heads on one key/value head, odd head counts, a last stretch of 2 queries
    (3, 4, 130, 10, 33, 8, 2, 128, False),
    (2, 3, 200, 7, 40, 3, 3, 256, False),
    (3, 5, 97, 9, 1, 6, 2, 128, False),
    (3, 4, 80, 10, 7, 4, 2, 256, False),      # 256-wide blocks below 96 tokens: the short kernel's two stretches
    # keys ending ONE past a 32-key chunk (a last chunk of one key, seen by one query)
    (5, 6, 44, 20, 21, 4, 4, 128, False),     # BASELINE's text-only layout: 21 prefix + 44 = 65 keys
    (4, 5, 33, 6, 0, 4, 2, 64, False),        # 33 keys, no prefix, grouped heads
    (3, 4, 33, 5, 64, 4, 4, 128, False),      # 97 keys
    (4, 6, 33, 7, 40, 2, 2, 128, True),       # 33 keys behind a prefix partial merged in the epilogue
    (3, 4, 65, 9, 32, 2, 1, 256, False),      # 256-wide heads, two stretches: the second ends at key 97 (64-query stretch + 1)
])
def test_ragged_attention_kernel_vs_fp32_loops(dtype, m, n_opt, L, T, P, H, Hk, Dh, merge):
    from bimodalattack_amd import ops
    from bimodalattack_amd.layout import ragged_plan
    rng = np.random.default_rng(1)
    parent = np.arange(n_opt)
    cand = np.tile(parent, (m, 1))
    for i in range(m):
        cand[i, rng.integers(0, n_opt)] = 100 + i
    plan = ragged_plan(cand, parent, L, T, P, n_opt + m * L - 3) or ragged_plan(cand, parent, L, T, P)
    N = plan["N"]
    g = torch.Generator(device=DEV).manual_seed(N)
    q, k, v = (torch.randn((N, hh, Dh), generator=g, device=DEV).to(dtype) for hh in (H, Hk, Hk))
    pk, pv = (torch.randn((max(P, 1), Hk, Dh), generator=g, device=DEV).to(dtype)[:P] for _ in range(2))
    scale = Dh ** -0.5
    ref = _ragged_attention_reference(q.float().cpu(), k.float().cpu(), v.float().cpu(), pk.float().cpu(),
                                      pv.float().cpu(), plan, P, scale)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    as4 = lambda t: t.unsqueeze(0).transpose(1, 2)                   # (1,heads,rows,Dh) view, rows strided
    args = (dev(plan["cstart"]), dev(plan["cfirst"]), dev(plan["clen"]), L, scale)
    if merge:
        s = torch.einsum("nhd,phd->hnp", q.float(), pk.float().repeat_interleave(H // Hk, 1)) * scale
        o1 = torch.einsum("hnp,phd->nhd", torch.softmax(s, -1), pv.float().repeat_interleave(H // Hk, 1)).to(dtype)
        got = ops.ragged_attention(as4(q), as4(k), as4(v), None, None, *args, o1=o1.contiguous(),
                                   lse1=torch.logsumexp(s, -1).contiguous())
    else:
        got = ops.ragged_attention(as4(q), as4(k), as4(v), as4(pk) if P else None, as4(pv) if P else None, *args)
    tol = 2e-2 if dtype == torch.bfloat16 else 3e-3
    assert got.shape == (N, H, Dh) and float((got.float().cpu() - ref).abs().max()) < tol


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,H,Hk,L,Dh,P", [(5, 8, 4, 303, 256, 20), (7, 4, 4, 44, 128, 21), (3, 4, 2, 65, 64, 0),
                                           (2, 2, 1, 17, 32, 128)])
def test_fused_block_attention_equals_sdpa(dtype, B, H, Hk, L, Dh, P):
    """Padded candidate blocks through the one-launch kernel (shared prefix + causal self attention, grouped
    heads in place) against torch's attention over the concatenated [prefix | own] sequence in fp32."""
    from bimodalattack_amd import prefix_attention as pa
    g = torch.Generator(device=DEV).manual_seed(B * L + P)
    # the projections' memory order is (B,L,heads,Dh); HF hands the attention function (B,heads,L,Dh) views
    q, k, v = (torch.randn((B, L, hh, Dh), generator=g, device=DEV).to(dtype).transpose(1, 2) for hh in (H, Hk, Hk))
    pk, pv = (torch.randn((1, max(P, 1), Hk, Dh), generator=g, device=DEV).to(dtype)[:, :P].transpose(1, 2) for _ in range(2))

    class KV:                                                  # the two things _fused_block_attention asks of the cache
        pass
    kv = KV()
    kv.P = P
    kv.prefix = lambda layer, n_rep: (pk, pv)
    scale = Dh ** -0.5
    got = pa._fused_block_attention(kv, 0, q, k, v, scale)
    assert got is not None and got.shape == (B, L, H, Dh)
    rep = H // Hk
    kk = torch.cat([pk.expand(B, -1, -1, -1), k], dim=2).float().repeat_interleave(rep, dim=1)
    vv = torch.cat([pv.expand(B, -1, -1, -1), v], dim=2).float().repeat_interleave(rep, dim=1)
    mask = torch.ones((L, P + L), dtype=torch.bool, device=DEV)
    mask[:, P:] = torch.tril(torch.ones((L, L), dtype=torch.bool, device=DEV))
    s_ = (q.float() @ kk.transpose(-1, -2)) * scale
    want = (torch.softmax(s_.masked_fill(~mask, float("-inf")), -1) @ vv).transpose(1, 2)
    tol = 2e-2 if dtype == torch.bfloat16 else 3e-3
    assert float((got.float() - want).abs().max()) < tol
    # a (B,heads,L,Dh) tensor that is NOT a view of (B,L,heads,Dh) memory is refused, not mis-read
    assert pa._fused_block_attention(kv, 0, q.contiguous(), k, v, scale) is None or H == 1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,P,H,Hk,Dh", [(300, 599, 8, 8, 128), (129, 70, 8, 4, 128), (17, 1, 4, 2, 64), (1000, 33, 16, 16, 64),
                                         (128, 32, 3, 3, 128)])
def test_prefix_attention_vs_fp32(dtype, N, P, H, Hk, Dh):
    """All rows against the shared prefix (no mask) on the matrix cores: output and natural-log LSE against
    fp32 softmax attention; row counts off the 128-row workgroup, prefix lengths off the 32-key chunk, grouped
    heads, a head count that is not a multiple of the XCD count."""
    from bimodalattack_amd import ops
    g = torch.Generator(device=DEV).manual_seed(N + P)
    q = torch.randn((1, N, H, Dh), generator=g, device=DEV).to(dtype).transpose(1, 2)          # (1,H,N,Dh) view
    pk, pv = (torch.randn((1, P, Hk, Dh), generator=g, device=DEV).to(dtype).transpose(1, 2) for _ in range(2))
    scale = Dh ** -0.5
    o, lse = ops.prefix_attention(q, pk, pv, scale)
    rep = H // Hk
    s_ = (q[0].float() @ pk[0].float().repeat_interleave(rep, 0).transpose(-1, -2)) * scale     # (H,N,P)
    want = (torch.softmax(s_, -1) @ pv[0].float().repeat_interleave(rep, 0)).transpose(0, 1)   # (N,H,Dh)
    tol = 2e-2 if dtype == torch.bfloat16 else 3e-3
    assert o.shape == (N, H, Dh) and float((o.float() - want).abs().max()) < tol
    np.testing.assert_allclose(lse.cpu().numpy(), torch.logsumexp(s_, -1).cpu().numpy(), rtol=2e-3, atol=2e-3)
    # the pair (o, lse) is what bma_ragged_attention merges: against the library's partial
    from bimodalattack_amd import prefix_attention as pa
    o_lib, lse_lib = pa._partial_attention(q, pk.repeat_interleave(rep, 1), pv.repeat_interleave(rep, 1), False, scale)
    assert float((o.float() - o_lib.transpose(1, 2)[0].float()).abs().max()) < 2 * tol
    np.testing.assert_allclose(lse.cpu().numpy(), lse_lib[0].cpu().numpy(), rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ragged_forward_equals_padded_forward(dtype):
    """Whole-model check on a small Llama: candidates that differ from a parent suffix from
    position p on, scored through the ragged row list, give the logits of the padded
    shared-prefix forward."""
    from bimodalattack_amd.hf_adapter import HFAdapter
    from bimodalattack_amd import ops, prefix_attention as pa, synthetic as S
    from bimodalattack_amd.layout import ragged_plan
    model = _small_llama(dtype)
    ad = HFAdapter(model, S.SyntheticProcessor(None), None)
    D = model.get_input_embeddings().weight.shape[1]
    m, P, n_opt, L, T = 9, 11, 6, 15, 4
    g = torch.Generator(device=DEV).manual_seed(21)
    prefix = (torch.randn((1, P, D), generator=g, device=DEV) * 0.5).to(dtype)
    table = (torch.randn((64, D), generator=g, device=DEV) * 0.5).to(dtype)            # "embeddings"
    rest = (torch.randn((1, L - n_opt, D), generator=g, device=DEV) * 0.5).to(dtype)    # after + target rows
    parent = np.arange(n_opt)
    cand = np.tile(parent, (m, 1))
    firsts = [0, 1, 2, 3, 4, 5, 5, 2, 0]
    for i, f in enumerate(firsts):
        cand[i, f] = 10 + i
    cand[6] = parent                                                                   # identical to the parent
    cand[8] = cand[1]                                                                  # an exact duplicate
    both = torch.from_numpy(np.concatenate([cand, parent[None]])).to(DEV)
    x = torch.cat([table[both], rest.expand(m + 1, -1, -1)], dim=1)                     # (m+1, L, D)
    n_rows = n_opt + sum(L - f for f in firsts)                                         # more than the 8 distinct need
    plan = ragged_plan(cand, parent, L, T, P, n_rows)
    assert plan is not None and plan["m"] == 8 and plan["m_out"] == m
    maps = pa.RaggedMaps(plan, DEV)
    mu = plan["m"]
    xu = torch.cat([table[torch.from_numpy(np.concatenate([plan["cand"], parent[None]])).to(DEV)],
                    rest.expand(mu + 1, -1, -1)], dim=1)                                # distinct candidates, plan order
    rows = ops.gather_rows(xu.view((mu + 1) * L, D).contiguous(), maps.flat).unsqueeze(0)
    with torch.no_grad():
        cache = ad.build_prefix_recording(prefix)
        want = ad.target_logits_shared_prefix(x[:m].contiguous(), T, cache).float()
        got = ad.target_logits_ragged(rows, T, cache, maps).float()
        # ... and with the engine's layer forward installed: the last layer's MLP on the m_out * T kept rows only
        from bimodalattack_amd.fused import FusedInference
        ad.fused = FusedInference(model)
        seen = []
        stack = next(mm for mm in model.modules() if isinstance(getattr(mm, "layers", None), torch.nn.ModuleList) and hasattr(mm, "norm"))
        hook = stack.layers[-1].mlp.register_forward_pre_hook(lambda mod, a: seen.append(tuple(a[0].shape)))
        with ad.fused:
            early = ad.target_logits_ragged(rows, T, cache, maps).float()
        hook.remove()
    assert got.shape == want.shape
    tol = 1e-4 if dtype == torch.float32 else 5e-2
    assert float((got - want).abs().max()) <= tol * max(1.0, float(want.abs().max()))
    assert seen == [(1, m * T, D)] and early.shape == want.shape
    assert float((early - want).abs().max()) <= tol * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("kind,dtype", [("llama", torch.float32), ("llama", torch.bfloat16), ("gemma3", torch.float32)])
def test_last_layer_runs_its_mlp_on_the_kept_rows_only(kind, dtype):
    """Scoring forwards read the target-predicting rows' logits only: with the engine's fused layer forward installed the
    rows are gathered right behind the LAST decoder layer's attention block (hf_adapter._logits_of_rows), so that layer's
    MLP and the final norm see T rows per candidate -- and the logits are those of the plain `logits_to_keep` call.  Three
    routes: the padded block with an HF cache, the shared-prefix block, the ragged row list (llama); under autograd, and
    outside the fused context, nothing is gathered early."""
    from bimodalattack_amd import hf_adapter, ops, prefix_attention as pa, synthetic as S
    from bimodalattack_amd.fused import FusedInference
    from bimodalattack_amd.hf_adapter import HFAdapter
    model = _small_llama(dtype) if kind == "llama" else S.tiny_case(kind, dtype=dtype, device=DEV)[0]
    ad = HFAdapter(model, S.SyntheticProcessor(None), None)
    fused = ad.fused = FusedInference(model)
    assert fused.admitted["last_layer_keeps_rows"] == 1
    D = model.get_input_embeddings().weight.shape[1]
    B, P, L, T = 6, 9, 12, 4
    g = torch.Generator(device=DEV).manual_seed(2)
    prefix = (torch.randn((1, P, D), generator=g, device=DEV) * 0.5).to(dtype)
    tail = (torch.randn((B, L, D), generator=g, device=DEV) * 0.5).to(dtype)
    stacks = [m for m in model.modules() if isinstance(getattr(m, "layers", None), torch.nn.ModuleList) and hasattr(m.layers[0], "mlp")
              and hasattr(m, "norm")]                   # (the text stack: the vision tower has no final `norm`)
    last_mlp, first_mlp = stacks[0].layers[-1].mlp, stacks[0].layers[0].mlp
    seen = {}
    hooks = [last_mlp.register_forward_pre_hook(lambda m, a: seen.setdefault("last", []).append(tuple(a[0].shape))),
             first_mlp.register_forward_pre_hook(lambda m, a: seen.setdefault("first", []).append(tuple(a[0].shape)))]
    tol = 1e-4 if dtype == torch.float32 else 5e-2

    def close(a, b):
        assert a.shape == b.shape
        assert float((a.float() - b.float()).abs().max()) <= tol * max(1.0, float(b.float().abs().max()))

    try:
        with torch.no_grad():
            cache = ad.build_prefix(prefix)
            with fused:
                hf_adapter.KEEP_ROWS_EARLY = False
                want = ad.target_logits(tail, T, cache=ad.expand_prefix(cache, B))
                assert seen["last"][-1] == (B, L, D)
                hf_adapter.KEEP_ROWS_EARLY = True
                got = ad.target_logits(tail, T, cache=ad.expand_prefix(cache, B))
                assert seen["last"][-1] == (B, T, D) and seen["first"][-1] == (B, L, D) and fused.keep_rows is None
                close(got, want)
                if ad.shared_prefix_configs():
                    rec = ad.build_prefix_recording(prefix)
                    got = ad.target_logits_shared_prefix(tail, T, rec)
                    assert seen["last"][-1] == (B, T, D)
                    close(got, want)
            # outside the context the layer forwards are HuggingFace's: the head's own gather
            got = ad.target_logits(tail, T, cache=ad.expand_prefix(cache, B))
            assert seen["last"][-1] == (B, L, D)
            close(got, want)
        # a forward that records a graph keeps every row (the gradient pass's row count is weight-bound anyway)
        with fused:
            xg = tail[:1].clone().requires_grad_()
            out = ad.target_logits(xg, T, cache=None)
            assert out.requires_grad and seen["last"][-1] == (1, L, D)
    finally:
        hf_adapter.KEEP_ROWS_EARLY = True
        for h in hooks:
            h.remove()


# ------------------------------------------------------------------ round 3: add + norm, q/k rotary, row-list splice
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("gemma", [False, True])
def test_add_rmsnorm_is_the_add_followed_by_the_norm(dtype, gemma):
    """bma_add_rmsnorm against the two launches it replaces -- aten's add, then bma_rmsnorm -- BIT for bit (sum and
    normed output), with and without the Gemma-3 sandwich norm on the addend; its autograd form against autograd
    through the separate Functions, bit for bit as well (the fused backward rounds where the accumulation would)."""
    from bimodalattack_amd import ops
    g = torch.Generator(device=DEV).manual_seed(31)
    sizes = ((65, 4096), (1000, 2560), (3, 128), (17, 8192 if dtype != torch.float32 else 4096))
    if dtype == torch.bfloat16:
        sizes += ((17152, 4096),)                       # the C3 candidate forward's row list at full size
    for rows, D in sizes:
        res = (torch.randn((1, rows, D), generator=g, device=DEV) * 3).to(dtype)
        h = (torch.randn((1, rows, D), generator=g, device=DEV) * 2).to(dtype)
        w = (torch.randn(D, generator=g, device=DEV) * 0.3 + (0.0 if gemma else 1.0)).to(dtype)
        wp = (torch.randn(D, generator=g, device=DEV) * 0.3 + (0.0 if gemma else 1.0)).to(dtype)
        s, y = ops.add_rmsnorm(res, h, w, 1e-6, gemma)
        s0 = res + h
        assert torch.equal(s, s0) and torch.equal(y, ops.rmsnorm(s0, w, 1e-6, gemma))
        s2, y2 = ops.add_rmsnorm(res, h, w, 1e-6, gemma, pre_weight=wp, pre_eps=1e-5)
        s3 = res + ops.rmsnorm(h, wp, 1e-5, gemma)
        y3 = ops.rmsnorm(s3, w, 1e-6, gemma)
        assert torch.equal(s2, s3)
        if dtype == torch.float16:
            # the three-in-one fp16 build differs from the separate launches by a unit or two in the last place on a few
            # outputs in ten thousand (a different, equally valid summation of the squares); the engine does not use it
            d = (y2.float() - y3.float()).abs()
            assert float((d > 0).float().mean()) < 1e-3 and bool((d <= 2.0 ** -9 * y3.float().abs() + 1e-6).all())
        else:
            assert torch.equal(y2, y3)
        # under autograd: d(res), d(h) with gradients arriving at BOTH outputs
        ds = torch.randn((1, rows, D), generator=g, device=DEV).to(dtype)
        dy = torch.randn((1, rows, D), generator=g, device=DEV).to(dtype)
        ra, ha = res.clone().requires_grad_(), h.clone().requires_grad_()
        sa, ya = ops.AddRMSNormFn.apply(ra, ha, w, 1e-6, gemma)
        ga = torch.autograd.grad([sa, ya], [ra, ha], [ds, dy])
        rb, hb = res.clone().requires_grad_(), h.clone().requires_grad_()
        sb = rb + hb
        yb = ops.RMSNormFn.apply(sb, w, 1e-6, gemma)
        gb = torch.autograd.grad([sb, yb], [rb, hb], [ds, dy])
        assert torch.equal(sa, sb) and torch.equal(ya, yb)
        for a_, b_ in zip(ga, gb):
            assert torch.equal(a_, b_)
        # only the normed output used downstream
        ra, ha = res.clone().requires_grad_(), h.clone().requires_grad_()
        (g1,) = torch.autograd.grad(ops.AddRMSNormFn.apply(ra, ha, w, 1e-6, gemma)[1], ra, dy)
        rb = res.clone().requires_grad_()
        (g2,) = torch.autograd.grad(ops.RMSNormFn.apply(rb + h, w, 1e-6, gemma), rb, dy)
        assert torch.equal(g1, g2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_rope2_is_two_ropes(dtype):
    """q and k rotated by one launch == the two one-tensor launches, bit for bit: grouped heads, the strided views of a
    fused q/k/v product, in place and out of place, forward and inverse."""
    from bimodalattack_amd import ops
    g = torch.Generator(device=DEV).manual_seed(5)
    for B, L, H, Hk, Dh in ((1, 65, 32, 32, 128), (3, 7, 8, 4, 256), (2, 44, 4, 2, 64)):
        qkv = torch.randn((B, L, (H + 2 * Hk) * Dh), generator=g, device=DEV).to(dtype)
        q = qkv[..., :H * Dh].view(B, L, H, Dh).transpose(1, 2)
        k = qkv[..., H * Dh:(H + Hk) * Dh].view(B, L, Hk, Dh).transpose(1, 2)
        ang = torch.randn((1, L, Dh // 2), generator=g, device=DEV)
        cos, sin = torch.cat([ang.cos()] * 2, -1).to(dtype), torch.cat([ang.sin()] * 2, -1).to(dtype)
        for inv in (False, True):
            q2, k2 = ops.rope2(q, k, cos, sin, inverse=inv)
            assert torch.equal(q2, ops.rope(q, cos, sin, inverse=inv)) and torch.equal(k2, ops.rope(k, cos, sin, inverse=inv))
        qa, ka = qkv.clone(), qkv.clone()
        q_in = qa[..., :H * Dh].view(B, L, H, Dh).transpose(1, 2)
        k_in = qa[..., H * Dh:(H + Hk) * Dh].view(B, L, Hk, Dh).transpose(1, 2)
        ops.rope2(q_in, k_in, cos, sin, inplace=True)
        ops.rope_(ka[..., :H * Dh].view(B, L, H, Dh).transpose(1, 2), cos, sin)
        ops.rope_(ka[..., H * Dh:(H + Hk) * Dh].view(B, L, Hk, Dh).transpose(1, 2), cos, sin)
        assert torch.equal(qa, ka)
        # autograd pair
        qg, kg = q.clone().requires_grad_(), k.clone().requires_grad_()
        dq, dk = torch.randn_like(q), torch.randn_like(k)
        a = torch.autograd.grad(ops.RoPE2Fn.apply(qg, kg, cos, sin), [qg, kg], [dq, dk])
        b = (torch.autograd.grad(ops.RoPEFn.apply(qg, cos, sin), qg, dq)[0], torch.autograd.grad(ops.RoPEFn.apply(kg, cos, sin), kg, dk)[0])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dtype,scale", [(torch.bfloat16, 1.0), (torch.float32, 1.0), (torch.bfloat16, 50.5)])
def test_splice_rows_is_splice_then_gather(dtype, scale):
    """bma_splice_rows (the ragged row list straight from the segments) == bma_splice + bma_gather_rows, byte for byte:
    shared, per-candidate and gathered segments, scaled embeddings, repeated and out-of-order slots."""
    from bimodalattack_amd import ops
    g = torch.Generator(device=DEV).manual_seed(17)
    B, n_opt, D, V = 37, 19, 512, 1000
    table = torch.randn((V, D), generator=g, device=DEV).to(dtype)
    ids = torch.randint(0, V, (B, n_opt), generator=g, device=DEV)
    segs = [("shared", torch.randn((1, 5, D), generator=g, device=DEV).to(dtype)), ("gather", None),
            ("percand", torch.randn((B, 3, D), generator=g, device=DEV).to(dtype)),
            ("shared", torch.randn((1, 20, D), generator=g, device=DEV).to(dtype))]
    S = 5 + n_opt + 3 + 20
    slot = torch.randint(0, B * S, (4000,), generator=g, device=DEV).to(torch.int32)
    slot[:S] = torch.arange(S, device=DEV, dtype=torch.int32) + (B - 1) * S          # the whole last block, in order
    want = ops.gather_rows(ops.splice(segs, B, table, ids, scale).view(B * S, D), slot)
    got = ops.splice(segs, B, table, ids, scale, rows=slot)
    assert got.shape == (4000, D) and torch.equal(got, want)


# ------------------------------------------------------------------ fused ops under autograd
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_backward_matches_eager_autograd(dtype):
    """dL/dx of the fused Functions against autograd through the eager HuggingFace modules.
    (The numerical bound, element by element against float64, is in tests/test_backward_gpu.py.)"""
    from bimodalattack_amd import ops
    from transformers.models.gemma3.modeling_gemma3 import Gemma3RMSNorm
    from transformers.models.llama.modeling_llama import LlamaRMSNorm, apply_rotary_pos_emb
    g = torch.Generator(device=DEV).manual_seed(9)
    tol = dict(rtol=2e-4, atol=2e-5) if dtype == torch.float32 else dict(rtol=5e-2, atol=5e-2)

    def close(a, b, what):
        a, b = a.float(), b.float()
        scale = float(b.abs().max()) + 1e-12
        assert float((a - b).abs().max()) <= tol["atol"] * scale + tol["rtol"] * scale, what

    rows, D = 65, 4096
    x = (torch.randn((1, rows, D), generator=g, device=DEV) * 2).to(dtype)
    dy = torch.randn((1, rows, D), generator=g, device=DEV).to(dtype)
    for gemma, cls in ((False, LlamaRMSNorm), (True, Gemma3RMSNorm)):
        m = cls(D, eps=1e-5).to(DEV, dtype)
        with torch.no_grad():
            m.weight.copy_((torch.randn(D, generator=g, device=DEV) * 0.3 + (0.0 if gemma else 1.0)).to(dtype))
        xe = x.clone().requires_grad_()
        (we,) = torch.autograd.grad(m(xe), xe, dy)
        xf = x.clone().requires_grad_()
        (wf,) = torch.autograd.grad(ops.RMSNormFn.apply(xf, m.weight, 1e-5, gemma), xf, dy)
        close(wf, we, f"rmsnorm gemma={gemma}")

    a = (torch.randn((1, rows, 11008), generator=g, device=DEV) * 2).to(dtype)
    b = torch.randn((1, rows, 11008), generator=g, device=DEV).to(dtype)
    d = torch.randn((1, rows, 11008), generator=g, device=DEV).to(dtype)
    ae, be = a.clone().requires_grad_(), b.clone().requires_grad_()
    ge = torch.autograd.grad(torch.nn.functional.silu(ae) * be, (ae, be), d)
    af, bf = a.clone().requires_grad_(), b.clone().requires_grad_()
    gf = torch.autograd.grad(ops.SwiGLUFn.apply(af, bf), (af, bf), d)
    close(gf[0], ge[0], "swiglu d_gate")
    close(gf[1], ge[1], "swiglu d_up")
    ae, be = a.clone().requires_grad_(), b.clone().requires_grad_()
    ge = torch.autograd.grad(torch.nn.functional.gelu(ae, approximate="tanh") * be, (ae, be), d)
    af, bf = a.clone().requires_grad_(), b.clone().requires_grad_()
    gf = torch.autograd.grad(ops.SwiGLUFn.apply(af, bf, ops.ACT_GELU_TANH), (af, bf), d)
    close(gf[0], ge[0], "geglu d_gate")
    close(gf[1], ge[1], "geglu d_up")

    B, L, H, Dh = 1, rows, 32, 128
    q = torch.randn((B, L, H * Dh), generator=g, device=DEV).to(dtype)
    ang = torch.rand((1, L, Dh // 2), generator=g, device=DEV) * 6.28
    emb = torch.cat([ang, ang], -1)
    cos, sin = emb.cos().to(dtype), emb.sin().to(dtype)
    dq = torch.randn((B, H, L, Dh), generator=g, device=DEV).to(dtype)
    qe = q.clone().requires_grad_()
    (re,) = torch.autograd.grad(apply_rotary_pos_emb(qe.view(B, L, H, Dh).transpose(1, 2), qe.view(B, L, H, Dh).transpose(1, 2), cos, sin)[0], qe, dq)
    qf = q.clone().requires_grad_()
    (rf,) = torch.autograd.grad(ops.RoPEFn.apply(qf.view(B, L, H, Dh).transpose(1, 2), cos, sin), qf, dq)
    close(rf, re, "rope")


def test_gradient_pass_fused_equals_eager_gradient():
    """The whole gradient pass on a small Llama: token gradient with the fused autograd ops
    against the eager HuggingFace backward (fp32: to 1e-4 of the gradient's scale)."""
    from bimodalattack_amd.fused import FusedInference
    model = _small_llama(torch.float32)
    D = model.get_input_embeddings().weight.shape[1]
    x = (torch.randn((1, 20, D), device=DEV) * 0.5)
    w = torch.randn((1, 20, 264), device=DEV)

    def grad(fused):
        xi = x.clone().requires_grad_()
        ctx = FusedInference(model, fused)
        with ctx:
            out = model(inputs_embeds=xi, use_cache=False).logits
        return torch.autograd.grad((out * w).sum(), xi)[0]

    ge, gf = grad(False), grad(True)
    assert float((ge - gf).abs().max()) <= 1e-4 * float(ge.abs().max())


def test_block_attention_at_gemma_size_properties():
    """The long-block attention kernel at BASELINE configs[4]'s full size (164 padded candidates of 303 tokens behind a
    20-key prefix, 8 query heads on 4 key/value heads, 256 wide) through size-independent properties: causality bit for
    bit, linearity in the values, and three whole blocks against fp32 attention over the concatenated sequence."""
    from bimodalattack_amd import ops
    B, L, P, H, Hk, Dh = 164, 303, 20, 8, 4, 256
    dt = torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(7)
    q = torch.randn((1, B * L, H, Dh), generator=g, device=DEV).to(dt).transpose(1, 2)
    k, v, v2 = (torch.randn((1, B * L, Hk, Dh), generator=g, device=DEV).to(dt).transpose(1, 2) for _ in range(3))
    pk, pv = (torch.randn((1, P, Hk, Dh), generator=g, device=DEV).to(dt).transpose(1, 2) for _ in range(2))
    cs = torch.arange(B, dtype=torch.int32, device=DEV) * L
    cf = torch.zeros(B, dtype=torch.int32, device=DEV)
    cl = torch.full((B,), L, dtype=torch.int32, device=DEV)
    scale = Dh ** -0.5
    run = lambda kk, vv, pvv=pv: ops.ragged_attention(q, kk, vv, pk, pvv, cs, cf, cl, L, scale).view(B, L, H, Dh)
    out = run(k, v)
    assert torch.isfinite(out.float()).all()
    # causality: keys and values behind position j do not touch the queries up to j -- not in the last bit
    j = 200
    k2, vv2 = k.clone(), v.clone()
    k2.view(1, Hk, B, L, Dh)[:, :, :, j + 1:] = torch.randn((1, Hk, B, L - j - 1, Dh), generator=g, device=DEV).to(dt) * 3
    vv2.view(1, Hk, B, L, Dh)[:, :, :, j + 1:] = torch.randn((1, Hk, B, L - j - 1, Dh), generator=g, device=DEV).to(dt) * 3
    out2 = run(k2, vv2)
    assert torch.equal(out[:, :j + 1], out2[:, :j + 1]) and not torch.equal(out[:, j + 1:], out2[:, j + 1:])
    # linearity in the values (the weights depend on q and k only): attn(v) + attn(v2) = attn(v + v2) up to bf16 rounding
    pv2 = torch.randn((1, P, Hk, Dh), generator=g, device=DEV).to(dt).transpose(1, 2)
    lhs = run(k, v).float() + run(k, v2, pv2).float()
    rhs = run(k, (v.float() + v2.float()).to(dt), (pv.float() + pv2.float()).to(dt)).float()
    assert float((lhs - rhs).abs().max()) < 6e-2 and float((lhs - rhs).abs().mean()) < 4e-3
    # eight whole blocks x 8 heads (64 (candidate, head) pairs, 303 queries each) against float64 attention over
    # [prefix | block] on the same bf16 operands: within 3 bf16 roundings of every row's own scale
    rep = H // Hk
    worst = 0.0
    for b in (0, 1, 40, 77, 100, 131, B - 2, B - 1):
        qb = q[0, :, b * L:(b + 1) * L].double()                                       # (H,L,Dh)
        kb = torch.cat([pk[0], k[0, :, b * L:(b + 1) * L]], dim=1).double().repeat_interleave(rep, dim=0)
        vb = torch.cat([pv[0], v[0, :, b * L:(b + 1) * L]], dim=1).double().repeat_interleave(rep, dim=0)
        mask = torch.ones((L, P + L), dtype=torch.bool, device=DEV)
        mask[:, P:] = torch.tril(torch.ones((L, L), dtype=torch.bool, device=DEV))
        s_ = (qb @ kb.transpose(-1, -2)) * scale
        want = (torch.softmax(s_.masked_fill(~mask, float("-inf")), -1) @ vb).transpose(0, 1)    # (L,H,Dh)
        worst = max(worst, _row_scale_err(out[b], want))
    assert worst <= 3 * 2.0 ** -8, worst


@pytest.mark.parametrize("plan", [1, 4, 8])
def test_prefix_attention_kernels_tails_and_grouped_heads(plan):
    """Both prefix kernels (bma_prefix_attention_set_plan: 1 = 16x16x32 products with 32-key chunks through registers,
    4 / 8 = 32x32x16 products with 32-key tiles by LDS-DMA on workgroups of 4 / 8 waves) against float64 attention on the
    same bf16 operands, within 3 bf16 roundings of every row's own scale: prefix lengths around the tile and ring sizes
    (one tile, a tile and one key, the four-tile ring and one more, a last tile of 1 / 23 / 31 / 32 keys), row counts off the
    workgroup sizes, grouped heads, strided key rows ((P, Hk, Dh) memory), values with a different scale per key so that
    a permuted key order inside a k-step would show."""
    from bimodalattack_amd import ops
    from bimodalattack_amd.native import lib
    dt, Dh = torch.bfloat16, 128
    scale = Dh ** -0.5
    try:
        lib.bma_prefix_attention_set_plan(plan)
        for N, P, H, Hk in [(130, 1, 4, 2), (257, 32, 8, 8), (200, 33, 8, 4), (300, 64, 2, 2), (131, 65, 8, 8), (400, 96, 4, 4),
                            (129, 127, 8, 2), (500, 128, 8, 8), (260, 129, 16, 16), (300, 160, 8, 8), (64, 161, 3, 3),
                            (1000, 599, 8, 8), (333, 640, 4, 4), (150, 1025, 8, 4)]:
            g = torch.Generator(device=DEV).manual_seed(7 * N + P)
            q = torch.randn((1, N, H, Dh), generator=g, device=DEV).to(dt).transpose(1, 2)
            pk, pv = (torch.randn((1, P, Hk, Dh), generator=g, device=DEV).to(dt).transpose(1, 2) for _ in range(2))
            pv = (pv.float() * torch.linspace(0.5, 2.0, P, device=DEV)[None, None, :, None]).to(dt)
            o, lse = ops.prefix_attention(q, pk, pv, scale)
            rep = H // Hk
            s_ = (q[0].double() @ pk[0].double().repeat_interleave(rep, 0).transpose(-1, -2)) * scale
            want = (torch.softmax(s_, -1) @ pv[0].double().repeat_interleave(rep, 0)).transpose(0, 1)
            assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
            worst = _row_scale_err(o, want)
            assert worst <= 3 * 2.0 ** -8, (plan, N, P, H, Hk, worst)
            np.testing.assert_allclose(lse.cpu().numpy(), torch.logsumexp(s_, -1).cpu().numpy(), rtol=2e-3, atol=2e-3)
    finally:
        lib.bma_prefix_attention_set_plan(0)


@pytest.mark.parametrize("plan", [1, 4])
def test_prefix_attention_running_maximum_under_adversarial_scores(plan):
    """The 32x32x16 kernel moves a query's running maximum only when a tile's maximum exceeds it by more than 2^4 after
    scaling (BMA_PA32_DEFER) and rescales its accumulators only then; random scores take the deferring path on almost every
    tile, so both paths are driven on purpose here (cdna_hip_programming.md T13: a passing check on bounded random data
    says nothing about the rare branch): scores that climb along the keys by a little per tile (deferred several times, then
    moved), by a lot per tile (moved every tile), that fall (never moved after the first tile), one late outlier key, and
    rows whose climbs differ inside one wave (some lanes move, others defer: the rescale is per lane, the skip per wave).
    Against float64 on the same bf16 operands; the 16x16x32 kernel (plan 1) takes the same data as the yardstick."""
    from bimodalattack_amd import ops
    from bimodalattack_amd.native import lib
    dt, Dh, N, P, H = torch.bfloat16, 128, 256, 599, 4
    scale = Dh ** -0.5
    g = torch.Generator(device=DEV).manual_seed(3)
    unit = torch.zeros(Dh, device=DEV)
    unit[0] = 1.0
    base_k = torch.randn((P, H, Dh), generator=g, device=DEV) * 0.05
    base_k[..., 0] = 0.0
    pv = torch.randn((1, P, H, Dh), generator=g, device=DEV).to(dt).transpose(1, 2)
    pos = torch.arange(P, device=DEV, dtype=torch.float32)
    ramps = {                                                         # score contribution of key j through dim 0, in log2 units
        "slow climb": 0.05 * pos,                                      # +1.6 per tile: deferred twice, then moved
        "fast climb": 0.4 * pos,                                       # +12.8 per tile: moved every tile
        "falling": -0.3 * pos,
        "late outlier": torch.where(pos == 570, torch.tensor(40.0, device=DEV), torch.zeros_like(pos)),
        "steps of 3.9 and 4.1": torch.floor(pos / 32) * torch.where(torch.floor(pos / 32) % 2 == 0, 3.9, 4.1),
    }
    try:
        lib.bma_prefix_attention_set_plan(plan)
        for name, ramp in ramps.items():
            k = base_k.clone()
            k[..., 0] = (ramp / (scale * 1.4426950408889634))[:, None]      # q[0] = 1 below: score = ramp in log2 units
            pk = k.unsqueeze(0).to(dt).transpose(1, 2)
            q = torch.randn((1, N, H, Dh), generator=g, device=DEV) * 0.5
            q[..., 0] = 1.0
            q[0, 1::2, :, 0] = 0.25                                       # odd rows climb a quarter as fast: lanes of one wave differ
            q = q.to(dt).transpose(1, 2)
            o, lse = ops.prefix_attention(q, pk, pv, scale)
            s_ = (q[0].double() @ pk[0].double().transpose(-1, -2)) * scale
            want = (torch.softmax(s_, -1) @ pv[0].double()).transpose(0, 1)
            assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all(), name
            worst = _row_scale_err(o, want)
            assert worst <= 3 * 2.0 ** -8, (plan, name, worst)
            np.testing.assert_allclose(lse.cpu().numpy(), torch.logsumexp(s_, -1).cpu().numpy(), rtol=2e-3, atol=2e-3, err_msg=name)
    finally:
        lib.bma_prefix_attention_set_plan(0)


def test_prefix_attention_at_joint_size_properties():
    """bma_prefix_attention at BASELINE configs[3]'s full size (17152 scoring rows against the 599 shared prefix keys,
    32 heads of 128): a row's result does not depend on which other rows are in the launch (bit for bit), linearity
    in the values, the LSE does not depend on the values, and 256 rows against fp32 attention."""
    from bimodalattack_amd import ops
    N, P, H, Dh = 17152, 599, 32, 128
    dt = torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(11)
    q = torch.randn((1, N, H, Dh), generator=g, device=DEV).to(dt).transpose(1, 2)
    pk, pv, pv2 = (torch.randn((1, P, H, Dh), generator=g, device=DEV).to(dt).transpose(1, 2) for _ in range(3))
    scale = Dh ** -0.5
    o, lse = ops.prefix_attention(q, pk, pv, scale)
    assert o.shape == (N, H, Dh) and torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    lo, hi = 3001, 4500                                                        # off the 128-row workgroup grid
    o_s, lse_s = ops.prefix_attention(q[:, :, lo:hi], pk, pv, scale)
    assert torch.equal(o_s, o[lo:hi]) and torch.equal(lse_s, lse[:, lo:hi])
    o2, lse2 = ops.prefix_attention(q, pk, pv2, scale)
    o12, lse12 = ops.prefix_attention(q, pk, (pv.float() + pv2.float()).to(dt), scale)
    assert torch.equal(lse, lse2) and torch.equal(lse, lse12)
    d = (o.float() + o2.float() - o12.float()).abs()
    assert float(d.max()) < 3e-2 and float(d.mean()) < 2e-3
    # 256 rows x 32 heads against float64 attention on the same bf16 operands: within 3 bf16 roundings of the row's own scale
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(3))[:256].to(DEV)
    s_ = (q[0, :, rows].double() @ pk[0].double().transpose(-1, -2)) * scale                    # (H,256,P)
    want = (torch.softmax(s_, -1) @ pv[0].double()).transpose(0, 1)
    worst = _row_scale_err(o[rows], want)
    assert worst <= 3 * 2.0 ** -8, worst
    np.testing.assert_allclose(lse[:, rows].cpu().numpy(), torch.logsumexp(s_, -1).cpu().numpy(), rtol=2e-3, atol=2e-3)


def test_ragged_attention_at_c3_size_properties():
    """bma_ragged_attention on the ragged row list of BASELINE configs[2] at full size (512 sampled candidates of a
    19-token suffix, 44-token blocks behind 21 shared prefix keys, 32 heads of 128): linearity in the values, changes
    to one candidate's own rows touch that candidate only (bit for bit), and five candidates against fp32 loops."""
    from bimodalattack_amd import ops
    from bimodalattack_amd.layout import ragged_plan
    m, n_opt, L, T, P, H, Dh = 512, 19, 44, 20, 21, 32, 128
    dt = torch.bfloat16
    rng = np.random.default_rng(0)
    parent = rng.integers(0, 32000, n_opt)
    cand = np.tile(parent, (m, 1))
    cand[np.arange(m), rng.integers(0, n_opt, m)] = rng.integers(0, 256, m) + 40000
    plan = ragged_plan(cand, parent, L, T, P)
    N = plan["N"]
    g = torch.Generator(device=DEV).manual_seed(5)
    q, k, v, v2 = (torch.randn((N, H, Dh), generator=g, device=DEV).to(dt) for _ in range(4))
    pk, pv, pv2 = (torch.randn((P, H, Dh), generator=g, device=DEV).to(dt) for _ in range(3))
    as4 = lambda t: t.unsqueeze(0).transpose(1, 2)
    cs, cf, cl = (torch.from_numpy(plan[n]).to(DEV) for n in ("cstart", "cfirst", "clen"))
    scale = Dh ** -0.5
    run = lambda kk, vv, pvv: ops.ragged_attention(as4(q), as4(kk), as4(vv), as4(pk), as4(pvv), cs, cf, cl, L, scale)
    out = run(k, v, pv)
    assert out.shape == (N, H, Dh) and torch.isfinite(out.float()).all()
    lhs = out.float() + run(k, v2, pv2).float()
    rhs = run(k, (v.float() + v2.float()).to(dt), (pv.float() + pv2.float()).to(dt)).float()
    assert float((lhs - rhs).abs().max()) < 6e-2 and float((lhs - rhs).abs().mean()) < 4e-3
    # one candidate's own rows (not the parent's: those are everybody's keys) changed: only its outputs move
    starts, lens = plan["cstart"].tolist(), plan["clen"].tolist()
    victim = next(i for i in range(len(starts) - 1, -1, -1) if starts[i] >= int(plan["cfirst"].max()))   # its rows are nobody's parent rows
    a0, a1 = starts[victim], starts[victim] + lens[victim]
    k2, vv2 = k.clone(), v.clone()
    k2[a0:a1] = torch.randn((a1 - a0, H, Dh), generator=g, device=DEV).to(dt)
    vv2[a0:a1] = torch.randn((a1 - a0, H, Dh), generator=g, device=DEV).to(dt)
    out2 = run(k2, vv2, pv)
    keep = torch.ones(N, dtype=torch.bool, device=DEV)
    keep[a0:a1] = False
    assert torch.equal(out[keep], out2[keep]) and not torch.equal(out[a0:a1], out2[a0:a1])
    # 16 candidates x 32 heads (512 (candidate, head) pairs) against float64 attention on the same bf16 operands, every query
    # row within 3 bf16 roundings of its own scale; five of them also against the fp32 loops the small cases are held to
    n_c = len(starts)
    pick = sorted({0, 1, 2, n_c // 7, n_c // 5, n_c // 4, n_c // 3, n_c // 2, n_c // 2 + 1, 2 * n_c // 3, 3 * n_c // 4, 4 * n_c // 5,
                   n_c - 4, n_c - 3, n_c - 2, n_c - 1})
    firsts = plan["cfirst"].tolist()
    worst = 0.0
    for i in pick:
        want = _ragged_candidate_reference64(q, k, v, pk, pv, starts[i], firsts[i], lens[i], P, scale)
        worst = max(worst, _row_scale_err(out[starts[i]:starts[i] + lens[i]], want))
    assert len(pick) >= 12 and worst <= 3 * 2.0 ** -8, worst
    five = [0, 1, n_c // 2, n_c - 2, n_c - 1]
    sub = dict(cstart=plan["cstart"][five], cfirst=plan["cfirst"][five], clen=plan["clen"][five])
    ref = _ragged_attention_reference(q.float().cpu(), k.float().cpu(), v.float().cpu(), pk.float().cpu(), pv.float().cpu(),
                                      sub, P, scale)
    for i in five:
        a, b = starts[i], starts[i] + lens[i]
        assert _row_scale_err(out[a:b].cpu(), ref[a:b].double()) <= 3 * 2.0 ** -8


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_qknorm_rope2_is_the_norm_followed_by_rope2(dtype):
    """bma_qknorm_rope2 against the two launches it replaces -- the per-head RMSNorm of q and k (bma_rmsnorm on the head
    rows), then bma_rope2 -- BIT for bit: Gemma-3's (1 + w) form and the plain one, grouped heads, the transposed views
    of separate projections, in place and out of place."""
    from bimodalattack_amd import ops
    g = torch.Generator(device=DEV).manual_seed(17)
    for B, L, H, Hk, Dh in ((3, 303, 8, 4, 256), (1, 65, 4, 4, 128), (2, 7, 6, 2, 64)):
        q = torch.randn((B, L, H, Dh), generator=g, device=DEV).to(dtype).transpose(1, 2)
        k = torch.randn((B, L, Hk, Dh), generator=g, device=DEV).to(dtype).transpose(1, 2)
        wq, wk = ((torch.randn(Dh, generator=g, device=DEV) * 0.3).to(dtype) for _ in range(2))
        ang = torch.randn((1, L, Dh // 2), generator=g, device=DEV)
        cos, sin = torch.cat([ang.cos()] * 2, -1).to(dtype), torch.cat([ang.sin()] * 2, -1).to(dtype)
        assert ops.qknorm_rope_ok(q) and ops.qknorm_rope_ok(k)
        for gemma in (True, False):
            qn = ops.rmsnorm(q.transpose(1, 2), wq, 1e-6, gemma).transpose(1, 2)
            kn = ops.rmsnorm(k.transpose(1, 2), wk, 1e-6, gemma).transpose(1, 2)
            want_q, want_k = ops.rope2(qn, kn, cos, sin)
            got_q, got_k = ops.qknorm_rope2(q, k, wq, wk, 1e-6, gemma, cos, sin)
            assert torch.equal(got_q, want_q) and torch.equal(got_k, want_k)
            q2, k2 = q.clone(memory_format=torch.preserve_format), k.clone(memory_format=torch.preserve_format)
            r = ops.qknorm_rope2(q2, k2, wq, wk, 1e-6, gemma, cos, sin, inplace=True)
            assert r[0] is q2 and torch.equal(q2, want_q) and torch.equal(k2, want_k)


def test_fused_context_defers_gemma_head_norms_into_the_rotation():
    """A small Gemma-3 text model under the fused context with and without `fuse_qk_rope`: the same logits bit for bit
    (the deferred q_norm / k_norm ride in bma_qknorm_rope2), nothing left pending, and with autograd the norms run on
    their own as before."""
    from transformers import Gemma3TextConfig
    from transformers.models.gemma3.modeling_gemma3 import Gemma3ForCausalLM
    from bimodalattack_amd.fused import FusedInference
    torch.manual_seed(0)
    cfg = Gemma3TextConfig(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                           num_key_value_heads=2, head_dim=64, sliding_window=512, max_position_embeddings=512)
    model = Gemma3ForCausalLM(cfg).to(DEV, torch.bfloat16).eval()
    ids = torch.randint(0, 512, (3, 40), device=DEV)
    on, off = FusedInference(model, fuse_qk_rope=True), FusedInference(model, fuse_qk_rope=False)
    assert len(on._rope_norms) == 4 and not off._rope_norms
    with torch.no_grad():
        with on:
            a = model(input_ids=ids).logits
            assert not on._pending
        with off:
            b = model(input_ids=ids).logits
    assert torch.equal(a, b)
    emb = model.get_input_embeddings()(ids).detach().requires_grad_()
    with on:
        ya = model(inputs_embeds=emb).logits
    (ga,) = torch.autograd.grad(ya.float().sum(), emb)
    emb2 = emb.detach().clone().requires_grad_()
    with off:
        yb = model(inputs_embeds=emb2).logits
    (gb,) = torch.autograd.grad(yb.float().sum(), emb2)
    assert torch.equal(ya, yb) and torch.equal(ga, gb)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_quick_gelu_is_the_eager_chain_bit_for_bit(dtype):
    """bma_quick_gelu and its backward against HuggingFace's QuickGELUActivation under autograd -- three aten kernels
    forward, five backward, each rounding to the dtype -- BIT for bit, at CLIP's MLP size and with extreme inputs."""
    from transformers.activations import QuickGELUActivation
    from bimodalattack_amd import ops
    g = torch.Generator(device=DEV).manual_seed(21)
    act = QuickGELUActivation()
    for shape, scale in (((1, 577, 4096), 3.0), ((3, 8), 1.0), ((2, 577, 4096), 40.0)):
        x = (torch.randn(shape, generator=g, device=DEV) * scale).to(dtype)
        if x.numel() >= 8:
            x.view(-1)[:8] = torch.tensor([0.0, -0.0, 1e4, -1e4, 88.0, -88.0, 1e-30, -3.0], device=DEV).to(dtype)
        dy = torch.randn(shape, generator=g, device=DEV).to(dtype)
        xa = x.clone().requires_grad_()
        ya = act(xa)
        (ga,) = torch.autograd.grad(ya, xa, dy)
        xb = x.clone().requires_grad_()
        yb = ops.QuickGELUFn.apply(xb)
        (gb,) = torch.autograd.grad(yb, xb, dy)
        same = lambda a, b: torch.equal(a.view(torch.int32 if dtype == torch.float32 else torch.int16),
                                        b.view(torch.int32 if dtype == torch.float32 else torch.int16))
        if dtype == torch.float32:
            # fp32: aten rounds nothing in between, but its compiler may contract differently: a few ulp
            np.testing.assert_allclose(yb.detach().cpu().numpy(), ya.detach().cpu().numpy(), rtol=2e-6, atol=1e-30)
            np.testing.assert_allclose(gb.cpu().numpy(), ga.cpu().numpy(), rtol=4e-6, atol=1e-30)
        else:
            assert same(yb.detach(), ya.detach()) and same(gb, ga)
        assert torch.equal(ops.quick_gelu(x), yb.detach())
    assert not ops.quick_gelu_ok(torch.zeros(8, device=DEV, dtype=torch.float16))      # fp16 keeps the eager chain


def test_tower_qkv_as_one_product_matches_the_three():
    """A small CLIP vision tower in bf16 with its q/k/v projections (weights and biases) run as ONE product and its
    QuickGELU as one launch (hf_adapter._fused_activations) against the untouched modules: features and pixel gradient
    within bf16 noise (another GEMM shape sums in another order), the patches gone afterwards, and a weight changed in
    place is noticed."""
    from transformers import CLIPVisionConfig, CLIPVisionModel
    from bimodalattack_amd.hf_adapter import HFAdapter
    torch.manual_seed(0)
    cfg = CLIPVisionConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=3, num_attention_heads=4,
                           image_size=112, patch_size=14, hidden_act="quick_gelu")
    tower = CLIPVisionModel(cfg).to(DEV, torch.bfloat16).eval()

    class Shell:                                   # the three things the two helpers ask of the adapter
        pass
    sh = Shell()
    sh.model, sh.device = tower, torch.device(DEV)
    sh.fuse_quick_gelu = sh.fuse_tower_qkv = True
    sh.fuse_tower_layernorm = False                 # (its own test below)
    sh._quick_gelus = sh._tower_attn = sh._proj_norms = sh._tower_layers = None
    for name in ("quick_gelu_modules", "tower_attention_modules", "projector_norms", "_tower_qkv_forwards", "_fused_activations",
                 "tower_layers", "_tower_layer_forward"):
        setattr(sh, name, getattr(HFAdapter, name).__get__(sh))
    assert len(sh.tower_attention_modules()) == 3 and len(sh.quick_gelu_modules()) == 3

    def run(fused):
        px = torch.randn((1, 3, 112, 112), generator=torch.Generator(device=DEV).manual_seed(1), device=DEV).to(torch.bfloat16).requires_grad_()
        ctx = sh._fused_activations() if fused else contextlib.nullcontext()
        with ctx:
            out = tower(pixel_values=px).last_hidden_state
        (g,) = torch.autograd.grad(out.float().pow(2).sum(), px)
        return out.detach().float(), g.float()
    import contextlib
    o0, g0 = run(False)
    o1, g1 = run(True)
    attn0 = next(m for m in tower.modules() if hasattr(m, "q_proj"))
    assert "forward" not in attn0.q_proj.__dict__
    assert float((o0 - o1).abs().max()) <= 3e-2 * float(o0.abs().max()) and float((g0 - g1).abs().max()) <= 5e-2 * float(g0.abs().max())
    with torch.no_grad():
        attn0.k_proj.weight.mul_(0.5)
    o2, _ = run(False)
    o3, _ = run(True)
    assert float((o2 - o3).abs().max()) <= 3e-2 * float(o2.abs().max()) and float((o2 - o0).abs().max()) > 1e-3


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_add_layernorm_forward_and_backward(dtype):
    """bma_add_layernorm / _bwd (round 5: CLIP's residual add + LayerNorm pairs, one launch each way) against float64 on the
    same operands -- the sum exactly the eager add's, the norm within one rounding of the dtype (plus the fp32 statistics'
    own error), the gradient within two -- and against the eager chain aten runs (add, F.layer_norm, autograd): equal up to
    one unit in the last place on a sliver of the elements (aten's Welford mean / variance differ from the two-pass ones in
    the last fp32 bits).  CLIP's 577 x 1024, a short row, four chunks per lane, one row; with and without the residual."""
    from bimodalattack_amd import ops
    g = torch.Generator(device=DEV).manual_seed(31)
    eps_dt = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -23}[dtype]
    for rows, D in ((577, 1024), (3, 8 if dtype != torch.float32 else 4), (5, 8192 if dtype != torch.float32 else 4096), (1, 1152)):
        r = torch.randn((rows, D), generator=g, device=DEV).to(dtype)
        h = (torch.randn((rows, D), generator=g, device=DEV) * 0.7 + 0.3).to(dtype)
        w = (1.0 + 0.2 * torch.randn(D, generator=g, device=DEV)).to(dtype)
        b = (0.1 * torch.randn(D, generator=g, device=DEV)).to(dtype)
        dy = torch.randn((rows, D), generator=g, device=DEV).to(dtype)
        ds = torch.randn((rows, D), generator=g, device=DEV).to(dtype)
        eps = 1e-5
        for with_res in (True, False):
            ra, ha = r.clone().requires_grad_(), h.clone().requires_grad_()
            if with_res:
                s_k, y_k = ops.AddLayerNormFn.apply(ra, ha, w, b, eps)
                gr_k, gh_k = torch.autograd.grad([s_k, y_k], [ra, ha], [ds, dy])
            else:
                y_k = ops.LayerNormFn.apply(ha, w, b, eps)
                (gh_k,) = torch.autograd.grad(y_k, ha, dy)
            # eager chain, the model dtype
            rb, hb = r.clone().requires_grad_(), h.clone().requires_grad_()
            s_e = rb + hb if with_res else hb
            y_e = torch.nn.functional.layer_norm(s_e, (D,), w, b, eps)
            if with_res:
                gr_e, gh_e = torch.autograd.grad([s_e, y_e], [rb, hb], [ds, dy])
                assert torch.equal(s_k.detach(), s_e.detach())                     # the sum: the eager add's bits
                assert torch.equal(gr_k, gh_k)                                       # one gradient for both inputs
            else:
                (gh_e,) = torch.autograd.grad(y_e, hb, dy)
            # float64 on the same (rounded) sum
            sd = s_e.detach().double().requires_grad_()
            yd = torch.nn.functional.layer_norm(sd, (D,), w.double(), b.double(), eps)
            (gd,) = torch.autograd.grad(yd, sd, dy.double())
            if with_res:
                gd = gd + ds.double()
            scale_y, scale_g = float(yd.abs().max()), float(gd.abs().max())
            assert float((y_k.detach().double() - yd.detach()).abs().max()) <= 1.1 * eps_dt * scale_y + 1e-6 * scale_y, (rows, D, with_res)
            assert float((gh_k.double() - gd).abs().max()) <= 2.2 * eps_dt * scale_g + 1e-5 * scale_g, (rows, D, with_res)
            # against aten: the same function, statistics summed in another order
            ne_y = float((y_k.detach() != y_e.detach()).float().mean())
            assert ne_y <= (0.02 if dtype != torch.float32 else 1.0), ne_y
            assert float((y_k.detach().double() - y_e.detach().double()).abs().max()) <= 1.1 * eps_dt * scale_y + 1e-6 * scale_y
            assert float((gh_k.double() - gh_e.double()).abs().max()) <= 2.2 * eps_dt * scale_g + 1e-5 * scale_g
            # no-grad form: the same bits as under autograd
            with torch.no_grad():
                s_n, y_n, _ = ops.add_layernorm(r if with_res else None, h, w, b, eps)
            assert torch.equal(y_n, y_k.detach()) and (not with_res or torch.equal(s_n, s_k.detach()))
    assert not ops.layernorm_ok(torch.zeros((2, 12), device=DEV, dtype=torch.bfloat16), torch.zeros(12, device=DEV, dtype=torch.bfloat16),
                                torch.zeros(12, device=DEV, dtype=torch.bfloat16))        # 24-byte rows


@pytest.mark.parametrize("kind", ["clip", "siglip"])
def test_tower_layers_with_add_and_layernorm_fused(kind):
    """A CLIP-L-shaped vision tower (1024 wide, 577 tokens, 3 layers) in bf16 with each residual add fused into the LayerNorm
    behind it -- inside a layer and across the layer boundary, forward and backward (hf_adapter._tower_layer_forward) -- against
    the untouched modules: hidden states of every layer and the pixel gradient within bf16 noise, the launches really on the
    kernel (2 per layer and direction, counted), the patches gone afterwards.  And a SigLIP-shaped one (Gemma-3's: 72-wide
    heads, 1024 tokens), whose patch embedding hands the first layer a TRANSPOSED view: the fused forward makes the residual
    stream contiguous once, or none of its layers would qualify."""
    import contextlib
    from transformers import CLIPVisionConfig, CLIPVisionModel, SiglipVisionConfig, SiglipVisionModel
    from bimodalattack_amd import ops
    from bimodalattack_amd.hf_adapter import HFAdapter, _clip_layer_ok
    torch.manual_seed(0)
    if kind == "clip":
        cfg = CLIPVisionConfig(hidden_size=1024, intermediate_size=4096, num_hidden_layers=3, num_attention_heads=16,
                               image_size=336, patch_size=14, hidden_act="quick_gelu")
        tower = CLIPVisionModel(cfg).to(DEV, torch.bfloat16).eval()
    else:
        cfg = SiglipVisionConfig(hidden_size=576, intermediate_size=1152, num_hidden_layers=3, num_attention_heads=8,
                                 image_size=448, patch_size=14, vision_use_head=False)
        tower = SiglipVisionModel(cfg).to(DEV, torch.bfloat16).eval()
    for p_ in tower.parameters():
        p_.requires_grad_(False)

    class Shell:
        pass
    sh = Shell()
    sh.model, sh.device = tower, torch.device(DEV)
    sh.fuse_quick_gelu = sh.fuse_tower_qkv = False
    sh.fuse_tower_layernorm = True
    sh._quick_gelus = sh._tower_attn = sh._proj_norms = sh._tower_layers = None
    for name in ("quick_gelu_modules", "tower_attention_modules", "projector_norms", "_tower_qkv_forwards", "_fused_activations",
                 "tower_layers", "_tower_layer_forward"):
        setattr(sh, name, getattr(HFAdapter, name).__get__(sh))
    layers = [m for m in tower.modules() if type(m).__name__ in ("CLIPEncoderLayer", "SiglipEncoderLayer")]
    assert len(layers) == 3 and len(sh.tower_layers()) == 3 and all(_clip_layer_ok(l) for l in layers)
    side = cfg.image_size
    calls = {"fwd": 0, "bwd": 0}
    keep_f, keep_b = ops.add_layernorm, ops._layernorm_bwd
    ops.add_layernorm = lambda *a, **k: (calls.__setitem__("fwd", calls["fwd"] + 1), keep_f(*a, **k))[1]
    ops._layernorm_bwd = lambda *a, **k: (calls.__setitem__("bwd", calls["bwd"] + 1), keep_b(*a, **k))[1]

    def run(fused):
        px = torch.randn((1, 3, side, side), generator=torch.Generator(device=DEV).manual_seed(1), device=DEV).to(torch.bfloat16).requires_grad_()
        ctx = sh._fused_activations() if fused else contextlib.nullcontext()
        with ctx:
            out = tower(pixel_values=px, output_hidden_states=True)
        hs = [t.detach().float() for t in out.hidden_states]
        (g,) = torch.autograd.grad(out.hidden_states[-2].float().pow(2).sum(), px)
        return hs, g.float()
    try:
        h0, g0 = run(False)
        assert calls == {"fwd": 0, "bwd": 0}
        h1, g1 = run(True)
    finally:
        ops.add_layernorm, ops._layernorm_bwd = keep_f, keep_b
    # forward: layer_norm1 of layer 0 alone, then (add + layer_norm2) and (add + next layer_norm1) per layer, the last layer's
    # second add in aten; backward: everything that feeds hidden_states[-2] -- the last layer does not
    assert calls["fwd"] == 1 + 2 * 3 - 1 and calls["bwd"] == 1 + 2 * 2, calls
    assert all("forward" not in l.__dict__ for l in layers)
    assert len(h0) == len(h1) == 4
    for a, b in zip(h0, h1):
        assert float((a - b).abs().max()) <= 3e-2 * float(a.abs().max())
    assert float((g0 - g1).abs().max()) <= 5e-2 * float(g0.abs().max())
    big = g0.abs() > 0.1 * g0.abs().max()
    assert float((torch.sign(g1[big]) == torch.sign(g0[big])).float().mean()) > 0.98
