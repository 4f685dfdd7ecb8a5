"""The L2-ball PGD image update on the MI355X: bma_l2_step / bma_apgd_l2_step against the torch restatement of
oracle/kernels.py bit for bit (image, state and norms), their determinism and graph capture, and whole runs with
``pgd_norm="l2"`` under both rules: every traced step replayed through the restatement, the routes of the step loop, host
reads, two ranks, and a full-size LLaVA-1.5-7B-shaped run.  The reference has no L2 update, so there is no golden."""

import os
import tempfile

import numpy as np
import pytest
import torch

from oracle.kernels import ULP, apgd_l2_restated, dist64, l2_restated, same_bits
from test_apgd_gpu import META5, META8, _HostReads, run_g8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(3 * 336 * 336, 0), (3 * 896 * 896, 0), (4097, 0), (4099, 0), (1023, 1), (5, 1), (3, 0)]


def _dev(a, offset=0):
    buf = torch.empty(a.size + offset, dtype=torch.float32, device=DEV)
    v = buf[offset:]
    v.copy_(torch.from_numpy(a))
    return v


def _inputs(n, seed=None):
    rs = np.random.RandomState(n if seed is None else seed)
    x0 = rs.uniform(0, 1, n).astype(np.float32)
    x = np.clip(x0 + rs.uniform(-0.25, 0.25, n), 0, 1).astype(np.float32)
    prev = np.clip(x0 + rs.uniform(-0.25, 0.25, n), 0, 1).astype(np.float32)
    best = rs.uniform(0, 1, n).astype(np.float32)
    g = rs.standard_normal(n).astype(np.float32)
    g[rs.choice(n, min(n, 4), replace=False)] = [0.0, -0.0, 1e-30, -1e-30][:min(n, 4)]
    return x, g, x0, prev, best


def _radii(n):
    """x lies about 0.14 * sqrt(n) from x0: a ball the step leaves (the projection scales) and one it cannot leave."""
    return 0.05 * float(np.sqrt(n)), 10.0 * float(np.sqrt(n)) + 1.0


# ------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("n,offset", SIZES)
def test_l2_kernel_equals_the_restatement_at_every_size(n, offset):
    """LLaVA's and Gemma-3's image sizes, tails of 1 and 3 behind the float4 body, views one float off the 16-byte grid
    (the scalar loop alone); ball active and idle, in place and out of place, a zero gradient, a NaN in the gradient."""
    from bimodalattack_amd import ops
    x, g, x0, _, _ = _inputs(n)
    sc = ops.L2Scratch(torch.device(DEV), n)
    active, idle = _radii(n)
    g_nan = g.copy()
    g_nan[n // 2] = np.nan
    for eps, alpha, grad, what in ((active, 0.5, g, "active"), (idle, 0.01, g, "idle"), (active, 0.5, np.zeros_like(g), "g=0"),
                                   (idle, 0.01, np.zeros_like(g), "g=0 idle"), (active, 0.5, g_nan, "nan")):
        want, wn = l2_restated(x, grad, x0, eps, alpha * eps)
        if n >= 1023 and what != "nan":                                   # the cases are what their names say
            assert (wn[1] > np.float32(eps)) == (what in ("active", "g=0")), (what, wn)
        for in_place in (False, True):
            xd = _dev(x, offset)
            out = ops.l2_step(xd, _dev(grad, offset), _dev(x0, offset), eps, alpha, out=xd if in_place else None, scratch=sc)
            assert (out.data_ptr() == xd.data_ptr()) == in_place
            assert same_bits(out.cpu().numpy(), want), (n, offset, what, in_place, "out")
            assert same_bits(sc.norms.cpu().numpy()[:2], wn), (n, offset, what, in_place, sc.norms.tolist(), wn.tolist())
        if what == "nan":
            assert np.isnan(want).all() and np.isnan(wn).all()
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,offset", SIZES)
def test_apgd_l2_kernel_equals_the_restatement_at_every_size(n, offset):
    from bimodalattack_amd import ops
    x, g, x0, prev, best = _inputs(n)
    sc = ops.L2Scratch(torch.device(DEV), n)
    active, idle = _radii(n)
    g_nan = g.copy()
    g_nan[n // 2] = np.nan
    for eps, grad, what in ((active, g, "active"), (idle, g, "idle"), (active, np.zeros_like(g), "g=0"), (active, g_nan, "nan")):
        eta = 2 * eps if what != "idle" else 0.01 * eps
        for take_best in (False, True):
            for restart in (False, True):
                for in_place in (False, True):
                    if in_place and what not in ("active", "idle"):
                        continue
                    xd, p, b = _dev(x, offset), _dev(prev, offset), _dev(best, offset)
                    sc.norms.fill_(-1.0)
                    out = ops.apgd_l2_step(xd, _dev(grad, offset), _dev(x0, offset), p, b, eps, eta, take_best, restart,
                                           out=xd if in_place else None, scratch=sc)
                    want = apgd_l2_restated(x, grad, x0, prev, best, eps, eta, take_best, restart)
                    key = (n, offset, what, take_best, restart, in_place)
                    for got, w, name in zip((out, p, b), want, ("out", "prev", "best")):
                        assert same_bits(got.cpu().numpy(), w), key + (name,)
                    norms = sc.norms.cpu().numpy()
                    if want[3] is None:                                    # the shortcut leaves the norms alone
                        assert norms.tolist() == [-1.0, -1.0, -1.0], key
                        continue
                    assert same_bits(norms, want[3]), key + (norms.tolist(), want[3].tolist())
                    if n >= 1023 and what in ("active", "idle"):
                        assert (want[3][1] > np.float32(eps)) == (what == "active"), key
                    if what == "nan":
                        assert np.isnan(want[0]).all() and np.isnan(norms).all()
    torch.cuda.synchronize()


@pytest.mark.parametrize("offset", [0, 1])
def test_l2_grid_stride_wrap_and_tail(offset):
    """More float4 groups than the 256 x 1024 lanes of the chain's grid and a tail of 3 behind them in the same launch; one
    float off the 16-byte grid the scalar loop takes all of it and wraps four times.  Both rules, and the copy-only call."""
    from bimodalattack_amd import ops
    n = 256 * 1024 * 4 + 4 * 1024 + 3
    x, g, x0, prev, best = _inputs(n)
    sc = ops.L2Scratch(torch.device(DEV), n)
    eps = _radii(n)[0]
    xd, gd, x0d = _dev(x, offset), _dev(g, offset), _dev(x0, offset)
    out = ops.l2_step(xd, gd, x0d, eps, 0.5, scratch=sc)
    want, wn = l2_restated(x, g, x0, eps, 0.5 * eps)
    assert same_bits(out.cpu().numpy(), want) and same_bits(sc.norms.cpu().numpy()[:2], wn)
    for take_best, restart in ((True, True), (False, True)):
        p, b = _dev(prev, offset), _dev(best, offset)
        out = ops.apgd_l2_step(xd, gd, x0d, p, b, eps, 2 * eps, take_best, restart, scratch=sc)
        want = apgd_l2_restated(x, g, x0, prev, best, eps, 2 * eps, take_best, restart)
        for got, w, name in zip((out, p, b), want, ("out", "prev", "best")):
            assert same_bits(got.cpu().numpy(), w), (offset, take_best, restart, name)
        if want[3] is not None:
            assert same_bits(sc.norms.cpu().numpy(), want[3]), (offset, take_best, restart)


def test_l2_kernels_are_deterministic():
    from bimodalattack_amd import ops
    n = 3 * 896 * 896
    x, g, x0, prev, best = _inputs(n, seed=3)
    eps = _radii(n)[0]
    sc = ops.L2Scratch(torch.device(DEV), n)
    xd, gd, x0d = _dev(x), _dev(g), _dev(x0)
    runs = []
    for _ in range(2):
        out = ops.l2_step(xd, gd, x0d, eps, 0.5, scratch=sc)
        a = (out.cpu().numpy(), sc.norms.cpu().numpy()[:2].copy())
        p, b = _dev(prev), _dev(best)
        out = ops.apgd_l2_step(xd, gd, x0d, p, b, eps, 2 * eps, True, False, scratch=sc)
        runs.append(a + (out.cpu().numpy(), p.cpu().numpy(), b.cpu().numpy(), sc.norms.cpu().numpy()))
    for u, v in zip(*runs):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))


def test_l2_wrappers_refuse_aliased_state_and_small_scratch():
    from bimodalattack_amd import ops
    x = torch.rand(64, device=DEV)
    p = x.clone()
    with pytest.raises(ValueError):
        ops.apgd_l2_step(x, x, x, p, p, 0.5, 1.0, False, False)
    with pytest.raises(ValueError):
        ops.apgd_l2_step(x, x, x, x, p.clone(), 0.5, 1.0, False, False)
    big = torch.rand(128, device=DEV)
    with pytest.raises(ValueError):
        ops.l2_step(big, big, big, 0.5, 0.1, scratch=ops.L2Scratch(torch.device(DEV), 64))
    e = torch.empty(0, device=DEV)
    assert ops.l2_step(e, e, e, 0.5, 0.1).numel() == 0


@pytest.mark.parametrize("rule", ["linf", "apgd"])
def test_l2_calls_are_graph_capturable(rule):
    """A step captured into a torch.cuda.graph and replayed on fresh inputs equals the eager call and the restatement."""
    from bimodalattack_amd import ops
    n = 3 * 336 * 336
    eps = _radii(n)[0]
    first, fresh = _inputs(n, seed=5), _inputs(n, seed=6)
    st = [_dev(a) for a in first]                       # x, g, x0, prev, best: the graph's static inputs
    out = torch.empty(n, dtype=torch.float32, device=DEV)
    sc = ops.L2Scratch(torch.device(DEV), n)

    def call(x, g, x0, prev, best, out, sc):
        if rule == "linf":
            return ops.l2_step(x, g, x0, eps, 0.5, out=out, scratch=sc)
        return ops.apgd_l2_step(x, g, x0, prev, best, eps, 2 * eps, True, False, out=out, scratch=sc)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(*st, out, sc)                              # warm: nothing lazy is left for the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(*st, out, sc)
    for t, a in zip(st, fresh):
        t.copy_(torch.from_numpy(a))
    out.zero_()
    sc.norms.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    got = [out.cpu().numpy(), st[3].cpu().numpy(), st[4].cpu().numpy(), sc.norms.cpu().numpy()]
    eager = [_dev(a) for a in fresh]
    sc2 = ops.L2Scratch(torch.device(DEV), n)
    e_out = call(*eager, torch.empty_like(out), sc2)
    if rule == "linf":
        want, wn = l2_restated(*fresh[:3], eps, 0.5 * eps)
        assert same_bits(got[0], want) and same_bits(got[3][:2], wn)
        assert same_bits(got[0], e_out.cpu().numpy()) and same_bits(got[3][:2], sc2.norms.cpu().numpy()[:2])
    else:
        want = apgd_l2_restated(*fresh, eps, 2 * eps, True, False)
        for a, b, c in zip(got, want, (e_out, eager[3], eager[4], sc2.norms)):
            assert same_bits(a, b) and same_bits(a, c.cpu().numpy())


# ------------------------------------------------------------------ whole runs
EPS, ALPHA = 4.0, 0.25          # tiny images: 2352 / 9408 pixels; the plain rule's step of 1.0 reaches the sphere in four steps
STEPS = {"linf": 12, "apgd": 40}


def run_l2(name, rule, over=None, trace=True, meta=None, **engine):
    over = dict(dict(eps=EPS, alpha=ALPHA, num_steps=STEPS[rule]), **(over or {}))
    engine.setdefault("pgd_norm", "l2")
    return run_g8(name, over, trace=trace, meta=meta, pgd_rule=rule, **engine)


def check_l2_trace(trace, res, eps, alpha, rule):
    """Every step's kernel output, state and norms equal the restatement applied to the engine's OWN recorded inputs; the
    host's flags equal ApgdState's logic applied to the engine's OWN losses.  Returns the steps that restarted."""
    from bimodalattack_amd.pgd import ApgdState
    restarts = []
    if rule == "linf":
        x0 = trace[0]["l2_x0"]
        for i, st in enumerate(trace):
            a = st["l2"]
            out, norms = l2_restated(a["x"], a["g"], x0, eps, alpha * eps)
            assert same_bits(a["out"], out.reshape(a["out"].shape)), f"step {i}: kernel output vs restatement"
            assert same_bits(st["image_after_pgd"], a["out"]), f"step {i}: the step's image is the kernel's output"
            assert same_bits(a["norms"][:2], norms), f"step {i}: norms {a['norms'].tolist()} vs {norms.tolist()}"
            if i:
                assert same_bits(a["x"], trace[i - 1]["image_after_pgd"]), f"step {i}: input is the last output"
        return restarts
    x0 = trace[0]["apgd_x0"]
    host = ApgdState(eps, "l2")
    for i, st in enumerate(trace):
        a = st["apgd"]
        cur = res.losses[i - 1] if i else None
        assert a["norm"] == "l2" and a["current_loss"] == cur, i
        assert (a["eta"], a["take_best"], a["restart"]) == host.decide(cur, i), f"step {i}: host flags"
        assert (a["eta_next"], a["count"], a["best_loss"]) == (host.eta, host.count, host.best_loss), f"step {i}: host state"
        out, prev, best, norms = apgd_l2_restated(a["x"], a["g"], x0, a["prev_in"], a["best_in"], eps, a["eta"],
                                                  a["take_best"], a["restart"])
        shape = a["out"].shape
        assert same_bits(a["out"], out.reshape(shape)), f"step {i}: kernel output vs restatement"
        assert same_bits(st["image_after_pgd"], a["out"]), f"step {i}: the step's image is the kernel's output"
        assert same_bits(a["prev_out"], prev.reshape(shape)) and same_bits(a["best_out"], best.reshape(shape)), f"step {i}: state"
        if norms is not None:
            assert same_bits(a["norms"], norms), f"step {i}: norms {a['norms'].tolist()} vs {norms.tolist()}"
        if i:
            assert same_bits(a["x"], trace[i - 1]["image_after_pgd"]), f"step {i}: input is the last output"
        if a["restart"]:
            restarts.append(i)
    return restarts


def check_feasible(image, x0, eps, norms, rule):
    """In [0,1] and in the ball, by a float64 recomputation and by the norms the last call left.  The projection's
    relative bound (test_pgd_l2.py) plus the rounding of the sum x0 + d*f, at most 2^-25 per pixel in the worst case."""
    image, x0 = np.asarray(image), np.asarray(x0)
    assert image.min() >= 0 and image.max() <= 1
    d = dist64(image, x0)
    slack = np.sqrt(image.size) * 2.0 ** -25
    assert d <= eps * (1 + 4 * ULP) + slack, (d, eps)
    last = float(norms[2] if rule == "apgd" else norms[1])       # the distance before the final projection
    assert np.isfinite(last) and d <= min(last, eps) * (1 + 4 * ULP) + slack, (d, last, eps)
    return d


@pytest.mark.parametrize("rule", ["linf", "apgd"])
@pytest.mark.parametrize("name", sorted(META8))
def test_l2_runs_replay_through_the_restatement(name, rule):
    m, res, trace, tmp = run_l2(name, rule)
    assert len(trace) == STEPS[rule] and np.isfinite(res.losses).all()
    restarts = check_l2_trace(trace, res, EPS, ALPHA, rule)
    last = trace[-1]["l2" if rule == "linf" else "apgd"]
    x0 = trace[0]["l2_x0" if rule == "linf" else "apgd_x0"]
    if rule == "apgd":
        assert restarts, "no restart: the run no longer reaches a halving"
    if not (rule == "apgd" and last["restart"] and not last["take_best"]):       # (the shortcut leaves stale norms)
        d = check_feasible(trace[-1]["image_after_pgd"], x0, EPS, last["norms"], rule)
        print(f"{name} {rule}: |x - x0| = {d:.6f} of {EPS}, restarts {restarts}, norms {last['norms'].tolist()}")
    assert sorted(os.listdir(tmp)) == sorted(f"{i}.png" for i in range(STEPS[rule]))      # save_images


@pytest.mark.parametrize("rule", ["linf", "apgd"])
@pytest.mark.parametrize("engine", [dict(gradient_ahead=False), dict(joint_winner_from_batch=False),
                                    dict(graph_gradient=False), dict(fuse_pgd_only=False)])
def test_l2_routes_agree(engine, rule):
    """The restructurings of the step loop off, one at a time: the same rule (every step replays), the same losses and the
    same final image as the default route.  The routes order the gradient pass's fp32 sums differently (rtol 1e-5 on the
    losses, as for the L-inf rules); a gradient off by 1e-5 relative moves a pixel by step * |u_i| * 1e-5 <= 1e-5 * step per
    step, so 12 steps of at most 2 * EPS stay within 1e-3 -- unless a checkpoint decision flips, which the flags check rules
    out by comparing them with the default route's."""
    name = "llava_pgd" if ("fuse_pgd_only" in engine or "graph_gradient" in engine) else "llava_joint"
    over = dict(num_steps=12)
    m, base, btrace, _ = run_l2(name, rule, over)
    m, res, trace, _ = run_l2(name, rule, over, **engine)
    check_l2_trace(trace, res, EPS, ALPHA, rule)
    np.testing.assert_allclose(res.losses, base.losses, rtol=1e-5)
    assert res.strings == base.strings
    if rule == "apgd":
        assert [(s["apgd"]["take_best"], s["apgd"]["restart"]) for s in trace] == \
            [(s["apgd"]["take_best"], s["apgd"]["restart"]) for s in btrace]
    diff = np.abs(trace[-1]["image_after_pgd"].astype(np.float64) - btrace[-1]["image_after_pgd"]).max()
    print(f"{name} {rule} {engine}: final images differ by at most {diff:.3e}")
    assert diff <= 1e-3


def test_linf_norm_given_explicitly_is_the_default_bit_for_bit():
    for rule, meta, name in (("linf", META5, "llava_pgd"), ("apgd", META8, "llava_joint")):
        a = run_g8(name, dict(num_steps=4), meta=meta, trace=False, pgd_rule=rule)
        b = run_g8(name, dict(num_steps=4), meta=meta, trace=False, pgd_rule=rule, pgd_norm="linf")
        assert a[1].losses == b[1].losses and a[1].strings == b[1].strings
        for i in range(4):
            assert open(os.path.join(a[3], f"{i}.png"), "rb").read() == open(os.path.join(b[3], f"{i}.png"), "rb").read()


def test_l2_in_a_gcg_only_run_changes_nothing():
    a = run_g8("llava_gcg", meta=META5, trace=False, pgd_rule="linf")
    for rule in ("linf", "apgd"):
        b = run_g8("llava_gcg", meta=META5, trace=False, pgd_rule=rule, pgd_norm="l2")
        assert a[1].losses == b[1].losses and a[1].strings == b[1].strings


@pytest.mark.parametrize("name", ["llava_pgd", "llava_joint", "llava_pgd_gcg"])
def test_l2_adds_no_host_reads(name):
    counts = {}
    over = dict(eps=EPS, alpha=ALPHA)
    for rule, norm in (("linf", "linf"), ("linf", "l2"), ("apgd", "linf"), ("apgd", "l2")):
        # (filter_first pinned: its automatic choice reads the host at steps that depend on the candidates, which the
        # different images change)
        kw = dict(trace=False, pgd_rule=rule, pgd_norm=norm, save_images=False, filter_first=False)
        run_g8(name, dict(over, num_steps=3), **kw)                                                   # warm
        with _HostReads() as h:
            run_g8(name, dict(over, num_steps=12), **kw)
        counts[(rule, norm)] = h.n
    assert len(set(counts.values())) == 1, counts


# ------------------------------------------------------------------ two ranks on one GPU
def _l2_rank_worker(rank, world, port, name, rule, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        out.put((rank,) + _run_with_state(name, rule))
    finally:
        dist.destroy_process_group()


def _run_with_state(name, rule):
    from bimodalattack_amd import BimodalAttackConfig, synthetic as S
    from bimodalattack_amd.attack import BimodalAttack
    from bimodalattack_amd.config import EngineOptions
    m = META8[name]
    model, tok, proc, image = S.tiny_case(m["kind"], device=DEV)
    cfg = BimodalAttackConfig(seed=1, verbosity="ERROR", optim_str_init=m["optim_str_init"], images_folder=tempfile.mkdtemp(),
                              **dict(m["config"], eps=EPS, alpha=ALPHA, num_steps=24))
    atk = BimodalAttack(model, tok, proc, cfg, S.Normalize(S.CLIP_MEAN, S.CLIP_STD),
                        EngineOptions.from_env(rng_device="cpu", strict=True, pgd_rule=rule, pgd_norm="l2"))
    res = atk.run(m["goal"], m["goal"], m["target"], image)
    a = atk.apgd_state
    state = () if a is None else (a.prev.cpu().numpy(), a.best.cpu().numpy(), (a.eta, a.best_loss, a.last_best, a.count))
    return (res.losses, res.strings, atk.final_image.detach().cpu().numpy(), atk.l2_scratch.norms.cpu().numpy()) + state


@pytest.mark.parametrize("rule", ["linf", "apgd"])
@pytest.mark.parametrize("name", ["llava_joint", "llava_pgd_gcg", "llava_pgd"])
def test_l2_two_ranks_equal_single(name, rule):
    import socket
    import torch.multiprocessing as mp
    single = _run_with_state(name, rule)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_l2_rank_worker, args=(r, 2, port, name, rule, out)) for r in range(2)]
    for p in procs:
        p.start()
    got = [out.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, losses, strings, img, norms, *state in got:
        assert strings == single[1], rank
        np.testing.assert_allclose(losses, single[0], rtol=1e-5)
        assert same_bits(img, single[2]), rank
        if rule == "apgd":
            assert state[2] == single[6], rank
            assert same_bits(state[0], single[4]) and same_bits(state[1], single[5]), rank
    r0, r1 = sorted(got, key=lambda t: t[0])
    assert r0[1:3] == r1[1:3] and same_bits(r0[3], r1[3]) and same_bits(r0[4], r1[4])


# ------------------------------------------------------------------ full size
def test_7b_l2_pgd_only_steps():
    """24 PGD-only steps of the synthetic LLaVA-1.5-7B with each rule in an L2 ball of radius 16 (the L-inf box of BASELINE
    configs[1], 64/255, has corners 146 away): every step replays, finite losses, the final image in the ball and the cube
    by the device's norms and by a float64 recomputation, no fast path given up."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import build_plugins
    from bimodalattack_amd import BimodalAttackConfig
    from bimodalattack_amd.attack import BimodalAttack
    from bimodalattack_amd.config import EngineOptions

    dev = torch.device(DEV)
    steps, eps, alpha = 24, 16.0, 0.125
    model, tok, proc, messages, goal, target, image, norm = build_plugins("pgd", dev, torch.bfloat16, 32)
    for rule in ("linf", "apgd"):
        cfg = BimodalAttackConfig(num_steps=steps, search_width=8, seed=1, verbosity="ERROR", pgd_attack=True,
                                  gcg_attack=False, eps=eps, alpha=alpha, images_folder=tempfile.mkdtemp())
        trace = []
        atk = BimodalAttack(model, tok, proc, cfg, norm,
                            EngineOptions.from_env(save_images=False, strict=True, pgd_rule=rule, pgd_norm="l2", trace=trace))
        res = atk.run(messages, goal, target, image.detach().clone())
        assert not atk.engine_state()["fallbacks"], atk.engine_state()["fallbacks"]
        assert np.isfinite(res.losses).all() and len(res.losses) == steps
        restarts = check_l2_trace(trace, res, eps, alpha, rule)
        last = trace[-1]["l2" if rule == "linf" else "apgd"]
        norms = atk.l2_scratch.norms.cpu().numpy()
        assert same_bits(norms[:len(last["norms"])], last["norms"])
        final = atk.final_image.detach().cpu().numpy()
        if not (rule == "apgd" and last["restart"] and not last["take_best"]):
            d = check_feasible(final, image.detach().cpu().numpy(), eps, norms, rule)
        else:
            d = dist64(final, image.detach().cpu().numpy())
            assert d <= eps * (1 + 4 * ULP) + np.sqrt(final.size) * 2.0 ** -25 and final.min() >= 0 and final.max() <= 1
        print(f"7B L2 {rule}, {steps} steps: |x - x0| = {d:.6f} of {eps}, norms {norms.tolist()}, restarts {restarts}, "
              f"losses {np.round(res.losses, 4).tolist()}")
