"""The sample-wise LTV all-pole filter at shapes OFF the ring grid (no ring width in {8,16,24,32,40} divides the hop, order
> 38, or a single frame): forward, carried-state forward and all three gradients of the wave-per-utterance kernels
(csrc/lpc_any.hip) against the float64 oracle.  Bar: <= 1e-4 relative (max-norm and L2), fp32 kernels.

The inputs are smooth reflection-coefficient tracks whose base logits have standard deviation ``scale``: at 0.5 the orders
>= 39 are not benign for ANY fp32 recursion (a numpy fp32 emulation of the sequential recursion, the transposed adjoint and
sequential correlation sums gives 2.8e-4 at M = 64, 6e-5 at M = 39-40), hence 0.25 there; with the scales below the same
emulation stays at or under 6e-6 for every case, more than 10 x inside the bar."""
import warnings

import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4


def dev(x):
    return torch.as_tensor(np.array(x, dtype=np.float32)).cuda()   # (a copy: the shared cases are read-only)


def smooth_case(B, F, M, hop, Tx=None, seed=0, walk=0.02, scale=0.5):
    from oracle import golf_oracle as O

    rng = np.random.default_rng(seed)
    logits = rng.normal(0, scale, (B, 1, M)) + np.cumsum(rng.normal(0, walk, (B, F, M)), 1)
    a = O.rc2lpc(np.tanh(logits)).astype(np.float32)
    gain = np.exp(-3 + np.cumsum(rng.normal(0, 0.05, (B, F)), 1)).astype(np.float32)
    Tx = (F - 1) * hop + 1 if Tx is None else Tx
    ex = rng.normal(0, 1, (B, Tx)).astype(np.float32)
    return ex, gain, a


def check(x, ref, what, tol=TOL):
    emax, el2 = rel_err(x, ref)
    print(f"{what}: rel-max {emax:.3e} rel-l2 {el2:.3e}")
    assert np.isfinite(x).all(), what
    assert emax <= tol and el2 <= tol, (what, emax, el2)


_cases = {}


def case(B, F, M, hop, Tx, scale):
    """Inputs, cotangent and the oracle's forward and gradients of one shape (computed once, never modified)."""
    key = (B, F, M, hop, Tx, scale)
    if key not in _cases:
        from golf_amd.functional import ss_output_length
        from oracle import golf_oracle as O

        ex, gain, a = smooth_case(B, F, M, hop, Tx=Tx, seed=B * 100 + F, scale=scale)
        T = ss_output_length(ex.shape[1], F, hop)
        gy = np.random.default_rng(1).normal(0, 1, (B, T)).astype(np.float32)
        ref = (O.ltv_allpole_ss_forward(ex, gain, a, hop),) + tuple(O.ltv_allpole_ss_backward(gy, ex, gain, a, hop))
        for v in (ex, gain, a, gy) + ref:
            v.setflags(write=False)
        _cases[key] = (ex, gain, a, gy, T, ref)
    return _cases[key]


def run(ex_t, gain_t, a_t, gy_t, hop):
    from golf_amd import functional as GF

    y = GF.ltv_allpole_ss(ex_t, gain_t, a_t, hop)
    (y * gy_t).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), ex_t.grad, gain_t.grad, a_t.grad


def leaves(ex, gain, a, grads=(True, True, True)):
    return tuple(dev(v).requires_grad_(g) for v, g in zip((ex, gain, a), grads))


@pytest.mark.parametrize("B,F,M,hop,Tx,scale", [
    (2, 9, 22, 100, None, 0.5),      # hop not a multiple of 8
    (3, 7, 22, 300, None, 0.5),      # 12.5 ms at 24 kHz
    (2, 12, 26, 220, None, 0.25),    # 10 ms at 22.05 kHz
    (2, 5, 40, 441, None, 0.25),     # order > 38, odd hop
    (2, 4, 39, 240, None, 0.25),     # first order past the grid at the recipe's hop
    (2, 5, 31, 256, None, 0.25),     # first order past the grid at hop 256
    (2, 6, 64, 96, None, 0.25),      # largest order; hop on the grid, order off it
    (2, 4, 64, 7, None, 0.25),       # hop << M: lanes spread over ten frames; T = 22 < M
    (1, 4, 5, 3, None, 0.5),         # hop < M, tiny
    (2, 200, 5, 1, None, 0.5),       # hop 1 (no interpolation)
    (1, 1, 4, 7, None, 0.5),         # F = 1: one output sample
    (3, 10, 22, 100, 777, 0.5),      # excitation ends inside a frame
    (3, 10, 22, 100, 1200, 0.5),     # excitation longer than (F-1)*hop+1: its tail's gradient is exactly 0
    (9, 4, 12, 50, None, 0.5),       # a batch that does not fill the last workgroup
    (2, 5, 1, 15, None, 0.5),        # M = 1
] + [(1, 20, 22, 16, Tx, 0.5) for Tx in (63, 64, 65, 129)])   # I/O-block edges (hop 16: no ring width for order 22)
def test_fwd_bwd_vs_oracle(B, F, M, hop, Tx, scale):
    ex, gain, a, gy, T, (r_y, r_ex, r_gain, r_a) = case(B, F, M, hop, Tx, scale)
    y, g_ex, g_gain, g_a = run(*leaves(ex, gain, a), dev(gy), hop)
    assert y.shape == (B, T) and g_ex.shape == ex.shape and g_gain.shape == gain.shape and g_a.shape == a.shape
    check(y.cpu().numpy(), r_y, "y")
    check(g_ex.cpu().numpy(), r_ex, "g_ex")
    check(g_gain.cpu().numpy(), r_gain, "g_gain")
    check(g_a.cpu().numpy(), r_a, "g_a")
    if ex.shape[1] > T:   # (the gradient buffer is NaN-poisoned before the backward: every zero here was written)
        assert torch.equal(g_ex[:, T:], torch.zeros_like(g_ex[:, T:]))


def test_partial_grads():
    ex, gain, a, gy, T, _ = case(2, 9, 22, 100, None, 0.5)
    full = run(*leaves(ex, gain, a), dev(gy), 100)[1:]
    for only in range(3):
        grads = run(*leaves(ex, gain, a, tuple(i == only for i in range(3))), dev(gy), 100)[1:]
        for i in range(3):
            if i == only:
                assert torch.equal(grads[i], full[i])
            else:
                assert grads[i] is None


def test_strided_rows():
    B, F, M, hop = 2, 9, 22, 100
    ex, gain, a, gy, T, (r_y, r_ex, r_gain, r_a) = case(B, F, M, hop, None, 0.5)
    wide = torch.zeros(B, T + 37, device="cuda")
    wide[:, 5:5 + T] = dev(ex)
    wide.requires_grad_(True)
    _, gain_t, a_t = leaves(ex, gain, a)
    gy_t = dev(np.ascontiguousarray(gy.T)).t()   # (B, T) with strides (1, B)
    assert not gy_t.is_contiguous()
    from golf_amd import functional as GF

    y = GF.ltv_allpole_ss(wide[:, 5:5 + T], gain_t, a_t, hop)
    y.backward(gy_t)
    torch.cuda.synchronize()
    check(y.detach().cpu().numpy(), r_y, "y")
    check(wide.grad[:, 5:5 + T].cpu().numpy(), r_ex, "g_ex")
    assert not wide.grad[:, :5].any() and not wide.grad[:, 5 + T:].any()
    check(gain_t.grad.cpu().numpy(), r_gain, "g_gain")
    check(a_t.grad.cpu().numpy(), r_a, "g_a")


def test_backward_is_reproducible():
    ex, gain, a, gy, T, _ = case(3, 7, 22, 300, None, 0.5)
    first = run(*leaves(ex, gain, a), dev(gy), 300)
    second = run(*leaves(ex, gain, a), dev(gy), 300)
    for u, v in zip(first, second):
        assert torch.equal(u, v)


@pytest.mark.parametrize("B,M,hop,F,entry", [(3, 40, 441, 12, True), (2, 64, 96, 20, False)])
def test_state_blocks_bitwise_offgrid(B, M, hop, F, entry):
    """Frame-aligned blocks chained through the state from zeros give the bits of the one-shot filter (last sample included);
    for one shape also the state entry from a random state against the float64 oracle with zi."""
    from golf_amd import functional as GF
    from oracle import golf_oracle as O

    ex, gain, a = smooth_case(B, F, M, hop, seed=B * 100 + F, scale=0.25)
    x, gain_t, a_t = dev(ex), dev(gain), dev(a)
    whole = GF.ltv_allpole_ss(x, gain_t, a_t, hop, mode="serial")
    rng = np.random.default_rng(B + M)
    st = torch.zeros(B, M, device="cuda")
    cuts = np.sort(rng.choice(np.arange(1, F - 1), size=6, replace=False))
    bounds = [0] + list(cuts) + [F - 1]
    parts = []
    for f0, f1 in zip(bounds[:-1], bounds[1:]):
        hi = f1 * hop + (1 if f1 == F - 1 else 0)
        parts.append(GF.ltv_allpole_ss_state(x[:, f0 * hop: hi], gain_t[:, f0: f1 + 1], a_t[:, f0: f1 + 1], hop, st))
    got = torch.cat(parts, 1)
    assert torch.equal(got, whole)
    assert torch.equal(st, whole.flip(1)[:, :M])
    if not entry:
        return
    F = 6
    T = (F - 1) * hop
    xs, gs, As = ex[:, :T], gain[:, :F], a[:, :F]
    zi = rng.normal(0, 0.3, (B, M)).astype(np.float32)
    st = dev(zi)
    y = GF.ltv_allpole_ss_state(dev(xs), dev(gs), dev(As), hop, st)
    torch.cuda.synchronize()
    A = np.stack([np.asarray(GF.linear_upsample(torch.tensor(As[..., i]).double(), hop))[:, :T] for i in range(M)], -1)
    G = np.asarray(GF.linear_upsample(torch.tensor(gs).double(), hop))[:, :T]
    ref = O.sample_wise_lpc(xs.astype(np.float64) * G, A, zi.astype(np.float64))
    check(y.cpu().numpy(), ref, "state entry")
    np.testing.assert_array_equal(st.cpu().numpy(), y.cpu().numpy()[:, ::-1][:, :M])
    Ts = 3   # a block shorter than M: y[-1-i] for i < T, then the old state shifted by T
    st2 = dev(zi)
    y2 = GF.ltv_allpole_ss_state(dev(xs[:, :Ts]), dev(gs[:, :2]), dev(As[:, :2]), hop, st2)
    expect = np.concatenate([y2.cpu().numpy()[:, ::-1], zi[:, : M - Ts]], 1)
    np.testing.assert_array_equal(st2.cpu().numpy(), expect)


def test_module_trains_at_offgrid_hop():
    from golf_amd import functional as GF
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import LTVMinimumPhaseFilterPrecise

    B, F, M, hop = 2, 6, 22, 300
    ex, gain, a, gy, T, (r_y, r_ex, r_gain, r_a) = case(B, F, M, hop, None, 0.5)
    filt = LTVMinimumPhaseFilterPrecise(lpc_order=M).cuda()
    ex_t, gain_t, a_t = leaves(ex, gain, a)
    gy_t = dev(gy)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        y = filt(AudioTensor(ex_t), AudioTensor(gain_t, hop), AudioTensor(a_t, hop)).as_tensor()
        (y * gy_t).sum().backward()
        torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.equal(y, GF.ltv_allpole_ss(dev(ex), dev(gain), dev(a), hop))
    check(y.detach().cpu().numpy(), r_y, "y")
    check(ex_t.grad.cpu().numpy(), r_ex, "g_ex")
    check(gain_t.grad.cpu().numpy(), r_gain, "g_gain")
    check(a_t.grad.cpu().numpy(), r_a, "g_a")
