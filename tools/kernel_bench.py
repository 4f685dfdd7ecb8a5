#!/usr/bin/env python3
"""Standalone driver for the hand-written kernels at BASELINE shapes.

    python tools/kernel_bench.py [--iters 20] [--only ce_rows,splice] [--json out.json]

Launches ONLY the libbma_hip kernels (no model), so it can run under
`rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (separate passes) to collect HBM
traffic for the roofline, and it times each kernel with the in-library HIP events.
Shapes: LLaVA-1.5-7B V=32064 D=4096 T=20 n_opt=19 sw=512; Gemma-3-4b
V=262208 D=2560.
"""

from __future__ import annotations

import argparse
import re
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from bimodalattack_amd import native, ops  # noqa: E402

DEV = "cuda:0"


def cases():
    g = torch.Generator(device=DEV).manual_seed(0)
    bf = torch.bfloat16

    def ce(B, T, V):
        x = (torch.randn((B, T, V), generator=g, device=DEV) * 2).to(bf)
        lab = torch.randint(0, V, (T,), generator=g, device=DEV)
        return lambda: ops.ce_target(x, lab)

    def ce_grad(T, V):
        x = (torch.randn((1, T, V), generator=g, device=DEV) * 2).to(bf)
        lab = torch.randint(0, V, (T,), generator=g, device=DEV)
        return lambda: ops.ce_target(x, lab, want_dlogits=True)

    def mellowmax(B, T, V, grad):
        # grad: both passes per call (the gather of B*T label elements, then B*T*V elements written); each pass has a
        # profile slot of its own, and the case reports the dlogits launch alone
        x = (torch.randn((B, T, V), generator=g, device=DEV) * 2).to(bf)
        lab = torch.randint(0, V, (T,), generator=g, device=DEV)
        out = torch.empty_like(x) if grad else None
        return lambda: ops.mellowmax_target(x, lab, 1.0, want_dlogits=grad, out=out)

    def margin(B, T, V, grad):
        # the row pass streams all B*T*V elements (ce_rows' bytes); grad: the write-only dlogits pass after it, which has a
        # profile slot of its own and is what the case reports
        x = (torch.randn((B, T, V), generator=g, device=DEV) * 2).to(bf)
        lab = torch.randint(0, V, (T,), generator=g, device=DEV)
        out = torch.empty_like(x) if grad else None
        return lambda: ops.margin_target(x, lab, 0.0, want_match=True, want_dlogits=grad, out=out)

    def token_dist(n_opt, V, D):
        # one pass over the whole table (V * D * 2 bytes) for up to 32 positions; the gradient in and the fp32 score out are
        # n_opt * V * 6 bytes beside it.  Also FMA-bound: n_opt * V * D subtract + FMA pairs on the fp32 vector pipe
        table = (torch.randn((V, D), generator=g, device=DEV) * 0.02).to(bf)
        grad = (torch.randn((n_opt, V), generator=g, device=DEV) * 0.01).to(bf)
        ids = torch.randint(0, V, (n_opt,), generator=g, device=DEV)
        out = torch.empty((n_opt, V), dtype=torch.float32, device=DEV)
        return lambda: ops.token_dist_score(grad, table, ids, 0.1, out=out)

    def splice(B, lens, D, V=32064, n_opt=19):
        table = torch.randn((V, D), generator=g, device=DEV).to(bf)
        ids = torch.randint(0, V, (B, n_opt), generator=g, device=DEV)
        segs = []
        for L in lens:
            segs.append(("gather", None) if L == "g" else ("shared", torch.randn((1, L, D), generator=g, device=DEV).to(bf)))
        out = torch.empty((B, sum(n_opt if L == "g" else L for L in lens), D), dtype=bf, device=DEV)
        return lambda: ops.splice(segs, B, table, ids, 1.0, out=out)

    def topk(rows, V, k=256, dtype=bf):
        gr = (torch.randn((rows, V), generator=g, device=DEV) * 0.01).to(dtype)
        mask = ops.build_mask_bits(torch.arange(0, 5), V, DEV)
        return lambda: ops.mask_topk(gr, mask, k)

    def linf(n):
        x0 = torch.rand(n, generator=g, device=DEV)
        x = x0.clone()
        gr = torch.randn(n, generator=g, device=DEV)
        return lambda: ops.linf_step(x, gr, x0, 64 / 255, 4 / 255, out=x)

    def apgd(n):
        # the steady-state call (no improvement, no checkpoint): 16 B read + 8 B written per pixel
        x0 = torch.rand(n, generator=g, device=DEV)
        x, prev, best = x0.clone(), x0.clone(), x0.clone()
        gr = torch.randn(n, generator=g, device=DEV)
        return lambda: ops.apgd_step(x, gr, x0, prev, best, 64 / 255, 2 * 64 / 255, False, False, out=x)

    def l2(n):
        # three passes (4 + 12 + 16 B per pixel); the figures printed are per PASS (launch), a call is launches / iters of them
        x0 = torch.rand(n, generator=g, device=DEV)
        x = x0.clone()
        gr = torch.randn(n, generator=g, device=DEV)
        sc = ops.L2Scratch(torch.device(DEV), n)
        return lambda: ops.l2_step(x, gr, x0, 16.0, 0.125, out=x, scratch=sc)

    def apgd_l2(n):
        # the steady-state call (no improvement, no checkpoint): four passes (4 + 12 + 16 + 24 B per pixel)
        x0 = torch.rand(n, generator=g, device=DEV)
        x, prev, best = x0.clone(), x0.clone(), x0.clone()
        gr = torch.randn(n, generator=g, device=DEV)
        sc = ops.L2Scratch(torch.device(DEV), n)
        return lambda: ops.apgd_l2_step(x, gr, x0, prev, best, 16.0, 32.0, False, False, out=x, scratch=sc)

    def scatter(B, n_opt=19, k=256):
        ids = torch.randint(0, 32000, (n_opt,), generator=g, device=DEV)
        tk = torch.randint(0, 32000, (n_opt, k), generator=g, device=DEV)
        rnd = torch.rand((B, n_opt), generator=g, device=DEV)
        rank = torch.randint(0, k, (B, 1), generator=g, device=DEV)

        def go():
            pos = ops.rand_positions(rnd, 1)
            return ops.sample_scatter(ids, tk, pos, rank)
        return go

    def rmsnorm(rows, D):
        x = torch.randn((rows, D), generator=g, device=DEV).to(bf)
        w = torch.randn((D,), generator=g, device=DEV).to(bf)
        return lambda: ops.rmsnorm(x, w, 1e-5)

    def swiglu(rows, I):
        a = torch.randn((rows, I), generator=g, device=DEV).to(bf)
        b = torch.randn((rows, I), generator=g, device=DEV).to(bf)
        return lambda: ops.swiglu(a, b)

    def rope(B, L, H, Dh):
        q = torch.randn((B, L, H * Dh), generator=g, device=DEV).to(bf).view(B, L, H, Dh).transpose(1, 2)
        ang = torch.rand((1, L, Dh), generator=g, device=DEV)
        cos, sin = ang.cos().to(bf), ang.sin().to(bf)
        return lambda: ops.rope_(q, cos, sin)

    def rope_qk(N, H, Hk, Dh):
        # q and k of one attention block in one launch, as strided views of a fused q/k/v product's output
        qkv = torch.randn((1, N, (H + 2 * Hk) * Dh), generator=g, device=DEV).to(bf)
        q = qkv[..., :H * Dh].view(1, N, H, Dh).transpose(1, 2)
        k = qkv[..., H * Dh:(H + Hk) * Dh].view(1, N, Hk, Dh).transpose(1, 2)
        ang = torch.rand((1, N, Dh), generator=g, device=DEV)
        cos, sin = ang.cos().to(bf), ang.sin().to(bf)
        return lambda: ops.rope2(q, k, cos, sin, inplace=True)

    def qknorm_rope(B, L, H, Hk, Dh):
        # Gemma-3 scoring: the per-head q/k norms inside the rotary launch, on the separate projections' outputs
        q = torch.randn((B, L, H, Dh), generator=g, device=DEV).to(bf).transpose(1, 2)
        k = torch.randn((B, L, Hk, Dh), generator=g, device=DEV).to(bf).transpose(1, 2)
        wq, wk = (torch.randn(Dh, generator=g, device=DEV).to(bf) for _ in range(2))
        ang = torch.rand((1, L, Dh), generator=g, device=DEV)
        cos, sin = ang.cos().to(bf), ang.sin().to(bf)
        return lambda: ops.qknorm_rope2(q, k, wq, wk, 1e-6, True, cos, sin, inplace=True)

    def merge(B, L, H, Dh):
        o1 = torch.randn((B, L, H, Dh), generator=g, device=DEV).to(bf)
        o2 = torch.randn((B, L, H, Dh), generator=g, device=DEV).to(bf)
        l1 = torch.randn((H, B * L), generator=g, device=DEV)
        l2 = torch.randn((B, H, L), generator=g, device=DEV)
        return lambda: ops.attn_merge(o1, o2, l1, l2)

    def rope_rows(N, H, Dh):
        # the ragged row list: one "sequence" of N rows, per-row rotary angles
        q = torch.randn((1, N, H * Dh), generator=g, device=DEV).to(bf).view(1, N, H, Dh).transpose(1, 2)
        ang = torch.rand((1, N, Dh), generator=g, device=DEV)
        cos, sin = ang.cos().to(bf), ang.sin().to(bf)
        return lambda: ops.rope_(q, cos, sin)

    def merge_rows(N, B2, L, H, Dh):
        o1 = torch.randn((N, H, Dh), generator=g, device=DEV).to(bf)
        o2 = torch.randn((B2, L, H, Dh), generator=g, device=DEV).to(bf)
        l1 = torch.randn((H, N), generator=g, device=DEV)
        l2 = torch.randn((B2, H, L), generator=g, device=DEV)
        rmap = torch.randperm(B2 * L, generator=g, device=DEV)[:N].sort().values.to(torch.int32)
        return lambda: ops.attn_merge_rows(o1, o2, l1, l2, rmap)

    def ragged_attn(m, n_opt, L, T, P, H, Dh):
        import numpy as np
        from bimodalattack_amd.layout import ragged_plan
        rng = np.random.default_rng(0)
        parent = rng.integers(0, 32000, n_opt)
        cand = np.tile(parent, (m, 1))
        cand[np.arange(m), rng.integers(0, n_opt, m)] = rng.integers(0, 256, m) + 40000
        plan = ragged_plan(cand, parent, L, T, P)
        N = plan["N"]
        q, k, v = (torch.randn((N, H, Dh), generator=g, device=DEV).to(bf).unsqueeze(0).transpose(1, 2) for _ in range(3))
        pk, pv = (torch.randn((P, H, Dh), generator=g, device=DEV).to(bf).unsqueeze(0).transpose(1, 2) for _ in range(2))
        cs, cf, cl = (torch.from_numpy(plan[n]).to(DEV) for n in ("cstart", "cfirst", "clen"))
        return lambda: ops.ragged_attention(q, k, v, pk, pv, cs, cf, cl, L, Dh ** -0.5)

    def block_attn(B, L, P, H, Hk, Dh):
        # padded candidate blocks (trivially ragged: first = 0, len = L) with grouped key/value heads: Gemma-3 joint
        q = torch.randn((1, B * L, H, Dh), generator=g, device=DEV).to(bf).transpose(1, 2)
        k, v = (torch.randn((1, B * L, Hk, Dh), generator=g, device=DEV).to(bf).transpose(1, 2) for _ in range(2))
        pk, pv = (torch.randn((1, P, Hk, Dh), generator=g, device=DEV).to(bf).transpose(1, 2) for _ in range(2))
        cs = torch.arange(B, dtype=torch.int32, device=DEV) * L
        cf = torch.zeros(B, dtype=torch.int32, device=DEV)
        cl = torch.full((B,), L, dtype=torch.int32, device=DEV)
        return lambda: ops.ragged_attention(q, k, v, pk, pv, cs, cf, cl, L, Dh ** -0.5)

    def gemm(M, N, K):
        # a library product of the candidate forward (hipBLASLt / rocBLAS through torch, with the shipped GEMM
        # selection when its validators match): not a bma kernel -- timed with torch events, PMC'd like the rest
        from bimodalattack_amd import gemm_tuning
        gemm_tuning.enable("auto", torch.device(DEV))
        x = torch.randn((1, M, K), generator=g, device=DEV).to(bf)
        w = (torch.randn((N, K), generator=g, device=DEV) * 0.02).to(bf)
        return lambda: torch.nn.functional.linear(x, w)

    def prefix_attn(N, P, H, Dh, plan=0):
        # plan: bma_prefix_attention_set_plan -- 0 by shape (128-wide heads: the 32x32x16 kernel), 1 the 16x16x32 kernel
        from bimodalattack_amd.native import lib
        q = torch.randn((1, N, H, Dh), generator=g, device=DEV).to(bf).transpose(1, 2)
        pk, pv = (torch.randn((1, P, H, Dh), generator=g, device=DEV).to(bf).transpose(1, 2) for _ in range(2))

        def run():
            lib.bma_prefix_attention_set_plan(plan)
            try:
                return ops.prefix_attention(q, pk, pv, Dh ** -0.5)
            finally:
                lib.bma_prefix_attention_set_plan(0)
        return run

    def prefix_attn_lib(N, P, H, Dh):
        # the library kernel the hand-written one replaces (aten efficient attention, no mask, with LSE)
        from bimodalattack_amd import prefix_attention as pa
        q = torch.randn((1, N, H, Dh), generator=g, device=DEV).to(bf).transpose(1, 2)
        pk, pv = (torch.randn((1, P, H, Dh), generator=g, device=DEV).to(bf).transpose(1, 2) for _ in range(2))
        return lambda: pa._partial_attention(q, pk, pv, False, Dh ** -0.5)

    def add_rmsnorm(rows, D):
        r = torch.randn((rows, D), generator=g, device=DEV).to(bf)
        h = torch.randn((rows, D), generator=g, device=DEV).to(bf)
        w = torch.randn((D,), generator=g, device=DEV).to(bf)
        return lambda: ops.add_rmsnorm(r, h, w, 1e-5)

    def splice_rows(m, n_opt, L, T, P, D, V=32064):
        # the ragged row list of C3 straight from the segments and the table (no padded block, no gather)
        import numpy as np
        from bimodalattack_amd.layout import ragged_plan
        rng = np.random.default_rng(0)
        parent = rng.integers(0, 32000, n_opt)
        cand = np.tile(parent, (m, 1))
        cand[np.arange(m), rng.integers(0, n_opt, m)] = rng.integers(0, 256, m) + 20000
        plan = ragged_plan(cand, parent, L, T, P)
        table = torch.randn((V, D), generator=g, device=DEV).to(bf)
        ids = torch.from_numpy(np.concatenate([plan["cand"], parent[None]])).to(DEV)
        flat = torch.from_numpy(plan["flat"]).to(DEV)
        segs = [("gather", None), ("shared", torch.randn((1, L - n_opt, D), generator=g, device=DEV).to(bf))]
        return lambda: ops.splice(segs, ids.shape[0], table, ids, 1.0, rows=flat)

    def gemm_nt(M, N, K, layers=8):
        # the skinny kernel over `layers` different weights (each launch streams its weight from HBM)
        ops.GEMM_NT_MIN_K_OVER_N = 0.0
        ops.gemm_workspace(torch.device(DEV))
        ops.gemm_workspace_for_graphs(torch.device(DEV))
        x = torch.randn((1, M, K), generator=g, device=DEV).to(bf)
        ws = [(torch.randn((N, K), generator=g, device=DEV) * 0.02).to(bf) for _ in range(layers)]
        state = {"i": 0}

        def go():
            state["i"] = (state["i"] + 1) % layers
            return ops.gemm_nt(x, ws[state["i"]])
        return go

    def gemm_mid(M, N, K, layers=8):
        # the 224-row-tile kernel over `layers` different weights (each launch streams its weight from HBM)
        ops.GEMM_MID_MIN_K_OVER_N = 0.0
        ops.gemm_workspace(torch.device(DEV))
        ops.gemm_workspace_for_graphs(torch.device(DEV))
        x = torch.randn((1, M, K), generator=g, device=DEV).to(bf)
        ws = [(torch.randn((N, K), generator=g, device=DEV) * 0.02).to(bf) for _ in range(layers)]
        state = {"i": 0}

        def go():
            state["i"] = (state["i"] + 1) % layers
            return ops.gemm_mid(x, ws[state["i"]])
        return go

    def b1_attn(S, H, backward):
        qkv = torch.randn((S, 3 * H * 128), generator=g, device=DEV).to(bf)
        ang = torch.rand((S, 64), generator=g, device=DEV) * 6.28
        cos, sin = torch.cat([ang.cos(), ang.cos()], -1).to(bf), torch.cat([ang.sin(), ang.sin()], -1).to(bf)
        out, lse = ops.b1_attention(qkv, cos, sin, H, 128 ** -0.5)
        dout = torch.randn((S, H * 128), generator=g, device=DEV).to(bf)
        if backward:
            return lambda: ops.b1_attention_bwd(qkv, cos, sin, out, lse, dout, H, 128 ** -0.5)
        return lambda: ops.b1_attention(qkv, cos, sin, H, 128 ** -0.5)

    def causal_attn(Lq, Lk, H, backward, Dh=128, causal=True):
        qkv = torch.randn((Lk, 3 * H * Dh), generator=g, device=DEV).to(bf)
        q = qkv[Lk - Lq:, :H * Dh].view(Lq, H, Dh)
        k = qkv[:, H * Dh:2 * H * Dh].view(Lk, H, Dh)
        v = qkv[:, 2 * H * Dh:].view(Lk, H, Dh)
        out, lse2 = ops.causal_attention(q, k, v, Dh ** -0.5, causal)
        dout = torch.randn((Lq, H, Dh), generator=g, device=DEV).to(bf)
        if backward:
            return lambda: ops.causal_attention_bwd(q, k, v, out, lse2, dout, Dh ** -0.5, causal=causal)
        return lambda: ops.causal_attention(q, k, v, Dh ** -0.5, causal)

    def gather(N, R, W):
        src = torch.randn((N, W), generator=g, device=DEV).to(bf)
        idx = torch.randint(0, N, (R,), generator=g, device=DEV).sort().values.to(torch.int32)
        return lambda: ops.gather_rows(src, idx)

    return {
        # name: (kernel id in the profiler, thunk factory)
        # ragged scoring of C3 (search_width 512, 19 suffix + 25 tail tokens): 17152 computed rows
        # (distinct candidates only), attention in one launch; the padded-block kernels below
        # (merge with a row map, row gather) serve fp32 models and heads the MFMA kernel does not take
        "rmsnorm/c3r_17152x4096": ("rmsnorm", lambda: rmsnorm(17152, 4096)),
        "swiglu/c3r_17152x11008": ("swiglu", lambda: swiglu(17152, 11008)),
        "rope/c3r_N17152_H32_Dh128": ("rope", lambda: rope_rows(17152, 32, 128)),
        "attn_merge/c3r_N17152_B481_L44": ("attn_merge", lambda: merge_rows(17152, 481, 44, 32, 128)),
        "ragged_attn/c3r_sw512_P21_L44_H32_Dh128": ("ragged_attn", lambda: ragged_attn(512, 19, 44, 20, 21, 32, 128)),
        "ragged_attn/gemma_B164_L303_P20_H8_Hk4_Dh256": ("ragged_attn", lambda: block_attn(164, 303, 20, 8, 4, 256)),
        "ragged_attn/c4_B512_L45_P0_H32_Dh128": ("ragged_attn", lambda: block_attn(512, 45, 0, 32, 32, 128)),
        # joint scoring: every computed row against the 599 shared prefix keys (168 GFLOP per launch)
        "prefix_attn/c4_N17152_P599_H32_Dh128": ("prefix_attn", lambda: prefix_attn(17152, 599, 32, 128)),
        "prefix_attn/c4_16x16x32_kernel_N17152_P599_H32_Dh128": ("prefix_attn", lambda: prefix_attn(17152, 599, 32, 128, plan=1)),
        "libattn/c4_17152x599x32x128": (None, lambda: prefix_attn_lib(17152, 599, 32, 128)),
        "gather_rows/c3r_21164_of_17152x4096": ("gather_rows", lambda: gather(17152, 481 * 44, 4096)),
        "rmsnorm/c3_22528x4096": ("rmsnorm", lambda: rmsnorm(22528, 4096)),
        "swiglu/c3_22528x11008": ("swiglu", lambda: swiglu(22528, 11008)),
        "rope/c3_B512_L44_H32_Dh128": ("rope", lambda: rope(512, 44, 32, 128)),
        "attn_merge/c4_B512_L45_H32_Dh128": ("attn_merge", lambda: merge(512, 45, 32, 128)),
        "rmsnorm/n8_2816x4096": ("rmsnorm", lambda: rmsnorm(2816, 4096)),
        "rmsnorm/head_391168x256": ("rmsnorm", lambda: rmsnorm(391168, 256)),
        "swiglu/n8_2816x11008": ("swiglu", lambda: swiglu(2816, 11008)),
        "ce_rows/llava_B512_T20_V32064": ("ce_rows", lambda: ce(512, 20, 32064)),
        "ce_rows/llava_B64_T20_V32064": ("ce_rows", lambda: ce(64, 20, 32064)),
        "ce_rows/gemma_B64_T20_V262208": ("ce_rows", lambda: ce(64, 20, 262208)),
        "ce_rows/gemma_B128_T20_V262208": ("ce_rows", lambda: ce(128, 20, 262208)),
        "ce_dlogits/llava_T20_V32064": ("ce_dlogits", lambda: ce_grad(20, 32064)),
        "mellowmax/loss_B512_T20_V32064": ("mellowmax", lambda: mellowmax(512, 20, 32064, False)),
        "mellowmax/dlogits_B512_T20_V32064": ("mellowmax_dlogits", lambda: mellowmax(512, 20, 32064, True)),
        "margin/loss_B512_T20_V32064": ("margin", lambda: margin(512, 20, 32064, False)),
        "margin/dlogits_B512_T20_V32064": ("margin_dlogits", lambda: margin(512, 20, 32064, True)),
        "margin/loss_B128_T20_V262208": ("margin", lambda: margin(128, 20, 262208, False)),
        "token_dist/llava_n20_V32064_D4096": ("token_dist", lambda: token_dist(20, 32064, 4096)),
        "token_dist/gemma_n20_V262208_D2560": ("token_dist", lambda: token_dist(20, 262208, 2560)),
        "splice/c3_tail_B512_S44_D4096": ("splice", lambda: splice(512, ["g", 6, 19], 4096)),
        "splice/c3_full_B512_S65_D4096": ("splice", lambda: splice(512, [21, "g", 6, 19], 4096)),
        "splice/c4_full_B64_S643_D4096": ("splice", lambda: splice(64, [5, 576, 18, "g", 6, 19], 4096)),
        "splice/c4_full_B512_S643_D4096": ("splice", lambda: splice(512, [5, 576, 18, "g", 6, 19], 4096)),
        "mask_topk/llava_19x32064_bf16": ("mask_topk", lambda: topk(19, 32064)),
        "mask_topk/gemma_19x262208_bf16": ("mask_topk", lambda: topk(19, 262208)),
        "mask_topk/llava_19x32064_f32": ("mask_topk", lambda: topk(19, 32064, dtype=torch.float32)),
        "linf/llava_3x336x336": ("linf", lambda: linf(3 * 336 * 336)),
        "linf/gemma_3x896x896": ("linf", lambda: linf(3 * 896 * 896)),
        "apgd/llava_3x336x336": ("apgd", lambda: apgd(3 * 336 * 336)),
        "apgd/gemma_3x896x896": ("apgd", lambda: apgd(3 * 896 * 896)),
        "l2/llava_3x336x336": ("l2", lambda: l2(3 * 336 * 336)),
        "l2/gemma_3x896x896": ("l2", lambda: l2(3 * 896 * 896)),
        "apgd_l2/llava_3x336x336": ("l2", lambda: apgd_l2(3 * 336 * 336)),
        "apgd_l2/gemma_3x896x896": ("l2", lambda: apgd_l2(3 * 896 * 896)),
        "sample_scatter/B512": ("sample_scatter", lambda: scatter(512)),
        # round 3: residual add + norm in one pass, the row list straight from the segments, the skinny weight-streaming product
        "rope/c3r_qk_N17152_H32_Dh128": ("rope", lambda: rope_qk(17152, 32, 32, 128)),
        "rope/gemma_qknorm_B160_L303_H8_Hk4_Dh256": ("rope", lambda: qknorm_rope(160, 303, 8, 4, 256)),
        "add_rmsnorm/c3r_17152x4096": ("add_rmsnorm", lambda: add_rmsnorm(17152, 4096)),
        "add_rmsnorm/n8_2816x4096": ("add_rmsnorm", lambda: add_rmsnorm(2816, 4096)),
        "splice/c3r_rows_17152_D4096": ("splice", lambda: splice_rows(512, 19, 44, 20, 21, 4096)),
        "gemm_nt/gate_up_dX_65x4096x22016": ("gemm_nt", lambda: gemm_nt(65, 4096, 22016)),
        "gemm_nt/qkv_dX_65x4096x12288": ("gemm_nt", lambda: gemm_nt(65, 4096, 12288)),
        "gemm_nt/gate_up_65x22016x4096": ("gemm_nt", lambda: gemm_nt(65, 22016, 4096)),
        "gemm_nt/down_65x4096x11008": ("gemm_nt", lambda: gemm_nt(65, 4096, 11008)),
        # round 4: the same products at 644 rows (the pass with the image in the prompt): MFMA work fed through L2 -> LDS
        "gemm_mid/gate_up_dX_644x4096x22016": ("gemm_mid", lambda: gemm_mid(644, 4096, 22016)),
        "gemm_mid/gate_up_644x22016x4096": ("gemm_mid", lambda: gemm_mid(644, 22016, 4096)),
        "gemm_mid/down_644x4096x11008": ("gemm_mid", lambda: gemm_mid(644, 4096, 11008)),
        # causal attention of the 643-token pass at batch 1 and of 44 rows behind a 599-key prefix: latency-bound (3.4 / 8.5 GFLOP)
        "causal_attn/fwd_L643_H32": ("causal_attn", lambda: causal_attn(643, 643, 32, False)),
        "causal_attn/bwd_L643_H32": ("causal_attn", lambda: causal_attn(643, 643, 32, True)),
        # SigLIP's tower in Gemma-3: 4096 tokens x 16 heads of 72, every key visible (77 GFLOP forward, 193 backward)
        "causal_attn/siglip_fwd_L4096_H16_D72": ("causal_attn", lambda: causal_attn(4096, 4096, 16, False, 72, False)),
        "causal_attn/siglip_bwd_L4096_H16_D72": ("causal_attn", lambda: causal_attn(4096, 4096, 16, True, 72, False)),
        # CLIP's tower in LLaVA: 577 tokens x 16 heads of 64
        "causal_attn/clip_fwd_L577_H16_D64": ("causal_attn", lambda: causal_attn(577, 577, 16, False, 64, False)),
        "causal_attn/clip_bwd_L577_H16_D64": ("causal_attn", lambda: causal_attn(577, 577, 16, True, 64, False)),
        "causal_attn/fwd_tail_L44_K643_H32": ("causal_attn", lambda: causal_attn(44, 643, 32, False)),
        "causal_attn/bwd_tail_L44_K643_H32": ("causal_attn", lambda: causal_attn(44, 643, 32, True)),
        # rotary + causal attention of the text-only gradient pass (65 rows, 32 heads of 128): latency-bound, one launch each way
        "b1_attn/fwd_S65_H32": ("b1_attn", lambda: b1_attn(65, 32, False)),
        "b1_attn/bwd_S65_H32": ("b1_attn", lambda: b1_attn(65, 32, True)),
        # the dominant kernel of a step: the fused gate/up product of the C3 ragged candidate forward
        "gemm/gate_up_17152x22016x4096": (None, lambda: gemm(17152, 22016, 4096)),
        "gemm/down_17152x4096x11008": (None, lambda: gemm(17152, 4096, 11008)),
        "gemm/qkv_17152x12288x4096": (None, lambda: gemm(17152, 12288, 4096)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    native.check_single_hip_runtime()
    want = [w for w in args.only.split(",") if w]
    results = {}
    all_cases = dict(cases())
    # calibration of the PMC byte counters on a KNOWN byte count (MI355X_MICROARCH.md, HBM: "calibrate on a known byte count
    # in your own access pattern"): a 256 MiB device-to-device copy -- reads 256 MiB, writes 256 MiB, 16 bytes per lane.
    # tools/make_profiles.py derives the FETCH_SIZE / WRITE_SIZE factors of the pass from this case.
    calib_src = torch.empty(128 << 20, dtype=torch.bfloat16, device=DEV).normal_()
    calib_dst = torch.empty_like(calib_src)
    all_cases = {"calib/copy_256MiB": ("calib", lambda: (lambda: calib_dst.copy_(calib_src))), **all_cases}
    for name, (kid, make) in all_cases.items():
        if want and not any(w in name for w in want) and kid != "calib":
            continue
        # a case marker in front of every case: a float64 reduction no case launches.  tools/pmc_traffic.py cuts the counter
        # rows at the markers, so that two cases that share a kernel symbol AND a grid (three gemm_nt shapes do) are never
        # averaged into one "run" -- the reason two round-4 entries read fewer bytes than their weights hold
        torch.zeros(4099, dtype=torch.float64, device=DEV).sum()
        fn = make()
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        if kid == "calib":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us = 1e3 * e0.elapsed_time(e1) / args.iters
            nbytes = 2.0 * calib_src.numel() * 2
            results[name] = dict(symbol="aten copy (16 B per lane)", launches=args.iters, avg_us=us, algorithmic_MB=nbytes / 1e6,
                                 read_MB=nbytes / 2e6, write_MB=nbytes / 2e6, achieved_GBps=nbytes / (us * 1e-6) / 1e9,
                                 frac_of_8TBps=nbytes / (us * 1e-6) / 8e12)
            print(f"{name:40s} {us:9.1f} us  {nbytes / 1e6:9.2f} MB  {nbytes / (us * 1e-6) / 1e9:8.0f} GB/s  (PMC calibration case)", flush=True)
            continue
        if kid is None:                       # a library GEMM: torch events on the current stream, flops not bytes
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us = 1e3 * e0.elapsed_time(e1) / args.iters
            dims = [int(v) for v in name.rsplit("_", 1)[1].split("x")]
            if len(dims) == 4:                # attention: rows x keys x heads x head dim
                M, N, K = dims[0] * dims[2], dims[1], 2 * dims[3]            # 4*N*P*Dh*H flops = 2*M*N*K
                mb = 2.0 * 2 * dims[0] * dims[2] * dims[3] / 1e6
            else:
                M, N, K = dims
                mb = 2.0 * (M * K + N * K + M * N) / 1e6
            tf = 2.0 * M * N * K / (us * 1e-6) / 1e12
            results[name] = dict(symbol="library GEMM", launches=args.iters, avg_us=us, algorithmic_MB=mb,
                                 algorithmic_GFLOP=2e-9 * M * N * K, achieved_TFLOPs=tf, frac_of_2500TFLOPs=tf / 2500.0,
                                 achieved_GBps=mb * 1e6 / (us * 1e-6) / 1e9, frac_of_8TBps=mb * 1e6 / (us * 1e-6) / 8e12)
            print(f"{name:40s} {us:9.1f} us  {mb:9.2f} MB  {tf:8.0f} TFLOP/s  {100 * tf / 2500.0:5.1f}% of 2.5 PFLOP/s", flush=True)
            del fn
            torch.cuda.empty_cache()
            continue
        native.profile_enable(True)
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        p = native.profile_read()[kid]
        native.profile_enable(False)
        us = 1e3 * p["ms"] / max(1, p["launches"])
        mb = p["bytes"] / max(1, p["launches"]) / 1e6
        gbs = p["bytes"] / (p["ms"] * 1e-3) / 1e9 if p["ms"] else 0.0
        results[name] = dict(symbol=p["symbol"], launches=p["launches"], avg_us=us, algorithmic_MB=mb,
                             achieved_GBps=gbs, frac_of_8TBps=gbs / 8000.0)
        extra = ""
        m = re.match(r"ragged_attn/\w+?_B(\d+)_L(\d+)_P(\d+)_H(\d+)(?:_Hk\d+)?_Dh(\d+)$", name)
        if m:                                 # padded blocks: causal flops = 4 * Dh * H * B * (L*P + L*(L+1)/2)
            B, L, P, H, Dh = (int(v) for v in m.groups())
            gf = 4.0 * Dh * H * B * (L * P + L * (L + 1) / 2) / 1e9
            tf = gf / 1e3 / (us * 1e-6)
            results[name].update(algorithmic_GFLOP=gf, achieved_TFLOPs=tf, frac_of_2500TFLOPs=tf / 2500.0)
            extra = f"  {gf:6.1f} GFLOP (causal) {tf:6.0f} TFLOP/s"
        m = re.match(r"gemm_mid/\w+?_(\d+)x(\d+)x(\d+)$", name)
        if m:                                 # MFMA work: 2 M N K flops
            M_, N_, K_ = (int(v) for v in m.groups())
            gf = 2.0 * M_ * N_ * K_ / 1e9
            tf = gf / 1e3 / (us * 1e-6)
            results[name].update(algorithmic_GFLOP=gf, achieved_TFLOPs=tf, frac_of_2500TFLOPs=tf / 2500.0)
            extra = f"  {gf:6.1f} GFLOP {tf:6.0f} TFLOP/s = {tf / 2500.0:4.2f} of the MFMA peak"
        if kid == "l2":                       # a call is a chain of launches: the sum of its passes beside the per-pass mean
            passes = p["launches"] // max(1, args.iters)
            results[name].update(passes_per_call=passes, call_us=us * passes, call_MB=mb * passes)
            extra = f"  per pass; x{passes} = {us * passes:.1f} us, {mb * passes:.2f} MB per call"
        print(f"{name:40s} {us:9.1f} us  {mb:9.2f} MB  {gbs:8.0f} GB/s  {100 * gbs / 8000.0:5.1f}% of 8 TB/s{extra}", flush=True)
        del fn
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
