"""The machinery the three target losses share (csrc/target_loss.hip) on the MI355X, on the smallest rows that pass
through every segment of the row walk: the head lane, the four-in-flight vector loop, the one-vector remainder loop and
the tail lane.  A row body of 1283 = 4*256 + 256 + 3 vectors sends lanes 0..2 through one unrolled trip and one remainder
trip and every other lane through the unrolled trip alone.  Each row holds one exactly tied pair of maxima that straddles
a border between two segments, so a first-index rule that is wrong at one border picks the wrong element there.

References: margin_ref.restated64 (bit for bit), oracle.kernels.ce_target, mellowmax_ref.restated64 with
mellowmax_ref.bounds -- the comparisons of test_margin_gpu.test_kernel_equals_the_restatement and
test_mellowmax_gpu.test_dlogits_every_element."""

import functools

import numpy as np
import pytest
import torch

import margin_ref as R
import mellowmax_ref as MM
import test_margin_gpu as MG
from oracle import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = MG.DTYPES
B, T, NVEC = 2, 3, 4 * 256 + 256 + 3
V_OFF = {4: 5137, 2: 10276}              # the one-element-off placement, by element size
KAPPA, GS, ALPHA = MG.KAPPA_GRID, 0.375, 1.0
LOW, HIGH = -5.0, 7.0                    # exact in every dtype


def row_split(ptr: int, V: int, es: int):
    """(head, nvec, tail) of a row of V elements at byte address `ptr`, as row_split in csrc/target_loss.hip."""
    ne = 16 // es
    head = min(V, ((16 - ptr % 16) & 15) // es)
    nvec = (V - head) // ne
    return head, nvec, head + nvec * ne


def placed(dtype, aligned: bool, fill: float):
    """((B,T,V) view, the flat buffer under it, the offset of the view): on the 16-byte grid with V = 1283 vectors, or one
    element into the buffer with ld_row = V off the grid."""
    es = torch.empty((), dtype=dtype).element_size()
    V, off = (NVEC * (16 // es), 0) if aligned else (V_OFF[es], 1)
    flat = torch.full((off + B * T * V + 9,), fill, dtype=dtype, device=DEV)
    assert flat.data_ptr() % 16 == 0
    return flat[off:off + B * T * V].view(B, T, V), flat, off


@functools.lru_cache(maxsize=None)
def case(dt: str, aligned: bool):
    """The block of one (dtype, placement), its labels and its float64 references, computed once."""
    dtype = DTYPES[dt]
    x, _, _ = placed(dtype, aligned, 30.0)                                       # (30: above every logit if ever read)
    es, V = x.element_size(), x.shape[2]
    ne = 16 // es
    z = np.full((B, T, V), LOW, np.float32)
    pairs, used = {}, set()
    for b in range(B):
        for t in range(T):
            head, nvec, tail = row_split(x.data_ptr() + (b * T + t) * V * es, V, es)
            assert nvec >= NVEC and (aligned or head or tail < V)
            mid = head + 4 * 256 * ne        # the first element of the remainder loop's vector; the one before it is the last
            borders = {"head": head, "mid": mid, "tail": tail}                   # of the unrolled trip's last vector
            want = ("head", "mid", "tail")[(b + t) % 3]
            if (want == "head" and head == 0) or (want == "tail" and tail == V):
                want = "mid"                 # a row with no head or tail uses the middle border
            first = borders[want] - 1
            z[b, t, first:first + 2] = HIGH
            pairs[b, t] = first
            used.add(want)
    assert used == ({"mid"} if aligned else {"head", "mid", "tail"})
    # over the rows of candidate 0: the label is the first of the pair, the second, neither
    lab = np.array([pairs[0, 0], pairs[0, 1] + 1, 5], np.int64)
    kinds = {int(lab[t] - pairs[b, t]) if 0 <= lab[t] - pairs[b, t] < 2 else -1 for b in range(B) for t in range(T)}
    assert kinds == {0, 1, -1}
    x.copy_(torch.from_numpy(z).to(dtype))
    assert torch.equal(x.float().cpu(), torch.from_numpy(z))
    assert x.data_ptr() % 16 == (0 if aligned else es) and (V * es % 16 == 0) == aligned      # the cross-entropy's VEC rule
    return dict(x=x, z=z, lab=lab, labd=torch.from_numpy(lab).to(DEV),
                margin=R.restated64(z, lab, KAPPA, grad_scale=GS, tie="first"), ce=K.ce_target(z, lab))


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "one_off"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_margin_at_the_segment_borders(dt, aligned):
    """m, i, match and dlogits bit-equal to the restatement; dlogits also into a block at the same placement."""
    from bimodalattack_amd import ops
    c = case(dt, aligned)
    x, ref = c["x"], c["margin"]
    loss, match, dlog, m = MG.check_call(x, c["lab"], c["labd"], KAPPA, ref, grid=True, gs=GS)
    ws = m._base.view(torch.int32).cpu().numpy().reshape(3, B, T)                # the scratch: m | i | row hit
    assert np.array_equal(ws[1], ref["i"]), (ws[1], ref["i"])
    assert np.array_equal(ws[2] != 0, c["z"].argmax(-1) == c["lab"][None])       # numpy's argmax: the first maximum
    out, flat, off = placed(x.dtype, aligned, 7.0)
    ops.margin_target(x, c["labd"], KAPPA, want_dlogits=True, grad_scale=GS, out=out)
    assert np.array_equal(MG.bits(out), MG.bits(dlog))
    assert (flat[:off] == 7.0).all() and (flat[off + out.numel():] == 7.0).all()


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "one_off"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_cross_entropy_at_the_segment_borders(dt, aligned):
    """The early-stop test equals the oracle's and the margin's, element for element; the loss within rtol 1e-5."""
    from bimodalattack_amd import ops
    c = case(dt, aligned)
    want, wmatch = c["ce"]
    loss, match, _, rows = ops.ce_target(c["x"], c["labd"], want_match=True)
    got = match.cpu().numpy()
    hits = rows._base[B * T:2 * B * T].view(torch.int32).cpu().numpy().reshape(B, T)        # the second third of the scratch
    assert np.array_equal(hits != 0, c["z"].argmax(-1) == c["lab"][None]) and hits.any() and not hits.all()
    print(f"{dt} aligned={aligned}: match {got}, worst relative loss error {np.abs(loss.cpu().numpy() / want - 1).max():.3e}")
    assert np.array_equal(got != 0, np.asarray(wmatch) != 0)
    assert torch.equal(match, ops.margin_target(c["x"], c["labd"], KAPPA, want_match=True)[1])
    np.testing.assert_allclose(loss.cpu().numpy(), want, rtol=1e-5)
    assert torch.equal(loss, ops.ce_target(c["x"], c["labd"])[0])                # the pass without the argmax: the same loss


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "one_off"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_mellowmax_dlogits_at_the_segment_borders(dt, aligned):
    """Every element of dlogits on the same blocks: +0 off the labels bit for bit, -w * grad_scale at them within the
    weight's bound plus one rounding of the dtype, nothing around the block touched."""
    from bimodalattack_amd import ops
    c = case(dt, aligned)
    x, lab = c["x"], c["lab"]
    out, flat, off = placed(x.dtype, aligned, 7.0)
    _, _, dlog, _ = ops.mellowmax_target(x, c["labd"], ALPHA, want_dlogits=True, grad_scale=GS, out=out)
    assert dlog.data_ptr() == out.data_ptr()
    assert (flat[:off] == 7.0).all() and (flat[off + out.numel():] == 7.0).all()
    at = np.zeros(out.shape, bool)
    at[:, np.arange(T), lab] = True
    assert (MG.bits(out)[~at] == 0).all()
    t = MM.gather_t(c["z"], lab)
    want = -MM.restated64(t, ALPHA)[1] * GS
    err = np.abs(out.float().cpu().numpy().astype(np.float64)[:, np.arange(T), lab] - want)
    bound = MM.bounds(t, ALPHA)[1] * GS + MM.ulp(want, x.dtype)
    print(f"{dt} aligned={aligned}: worst label error / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), (err, bound)
