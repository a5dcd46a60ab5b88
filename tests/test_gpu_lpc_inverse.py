"""GPU parity of the inverse (analysis) filter golf_ltv_inverse_{f32,bwd_f32} (csrc/lpc_ss.hip; behind GF.ltv_inverse,
LTVMinimumPhaseFilter*.reverse and the residual of LPCAnalysis) at any hop and any order up to 64: values and both gradients
against the float64 oracle (ltv_inverse_filter / ltv_inverse_backward, pinned by goldens g5 and g17), at the bound of the
full-size test in tests/test_gpu_lpc_ss.py."""
import numpy as np
import pytest
import torch

import parity
from parity import dev

pytestmark = pytest.mark.gpu

TOL = 2e-5
WORST = parity.Worst("ltv_inverse")


def _inputs(B, F, M, Ty, seed):
    rng = np.random.default_rng(seed)
    y = rng.normal(0, 1, (B, Ty)).astype(np.float32)
    a = (rng.normal(0, 1, (B, F, M)) * 0.5 / np.sqrt(M)).astype(np.float32)
    ge = rng.normal(0, 1, (B, Ty)).astype(np.float32)           # cut to the output's length where the input is clipped
    return y, a, ge


def _run(y, a, ge, hop, need_y=True, need_a=True):
    from golf_amd import functional as GF

    yt, at = dev(y, need_y), dev(a, need_a)
    e = GF.ltv_inverse(yt, at, hop)
    (e * dev(ge[:, : e.shape[1]])).sum().backward()
    torch.cuda.synchronize()
    return (e.detach().cpu().numpy(), yt.grad.cpu().numpy() if need_y else None, at.grad.cpu().numpy() if need_a else None)


def _check(what, got, y, a, ge, hop):
    from oracle import golf_oracle as O

    ref = O.ltv_inverse_filter(y, a, hop)
    assert got[0].shape == ref.shape
    rgy, rga = O.ltv_inverse_backward(ge[:, : ref.shape[1]], y, a, hop)
    for g, r, name in zip(got, (ref, rgy, rga), ("e", "g_y", "g_a")):
        if g is not None:
            parity.check_global(WORST, f"{what} {name}", g, r, TOL)
    return ref, rgy, rga


# (B, F, M, hop, T, trailing frames whose interpolation touches no sample)
CASES = [
    (2, 6, 64, 1, 6, 0),          # hop 1 (w = 0 everywhere), order above the length: every tap loop breaks early
    (2, 9, 33, 3, 25, 0),         # hop far below the order: one sample's taps reach back over 11 segments
    (1, 2, 64, 500, 501, 0),      # one segment, hop above the g_a wave's stride of 64 (8 strides per lane), clamped tail
    (3, 5, 1, 7, 29, 0),          # order 1
    (2, 7, 40, 16, 70, 1),        # T ends inside segment 4: trailing frame 6 has no sample
    (2, 3, 64, 300, 130, 1),      # T ends inside segment 0: trailing frame 2 has no sample
    (2, 4, 22, 240, 721, 0),      # the recipe's hop and order, the clamped tail sample (t = 720, w = 1 on the last frame)
    (2, 12, 17, 5, 56, 0),        # odd order, odd hop, full length
]


@pytest.mark.parametrize("B,F,M,hop,T,n_dead", CASES)
def test_inverse_any_hop_any_order_vs_oracle(B, F, M, hop, T, n_dead):
    y, a, ge = _inputs(B, F, M, T, 100 * M + hop)
    got = _run(y, a, ge, hop)
    _, _, rga = _check(f"inverse B{B} F{F} M{M} hop{hop} T{T}", got, y, a, ge, hop)
    if n_dead:
        dead = F - n_dead                                    # first frame whose interpolation touches no sample
        assert dead == (T - 1) // hop + 2
        assert np.all(rga[:, dead:] == 0.0) and np.all(got[2][:, dead:] == 0.0)
        assert np.all(np.abs(got[2][:, dead - 1]).max(-1) > 0.0)


def test_inverse_single_frame():
    """F = 1: constant coefficients, the output is one sample long (e[0] = y[0]; no tap reaches a sample)."""
    y, a, ge = _inputs(3, 1, 22, 1, 7)
    got = _run(y, a, ge, 240)
    _check("inverse F1", got, y, a, ge, 240)
    assert np.array_equal(got[0], y) and np.array_equal(got[1], ge) and np.all(got[2] == 0.0)


def test_inverse_clips_a_longer_input():
    """An input longer than (F-1)*hop + 1 is clipped to it, and g_y beyond is exactly 0."""
    B, F, M, hop = 2, 4, 30, 12
    T = (F - 1) * hop + 1
    y, a, ge = _inputs(B, F, M, T + 19, 8)
    got = _run(y, a, ge, hop)
    assert got[0].shape == (B, T) and got[1].shape == (B, T + 19)
    _check("inverse clipped", got, y, a, ge, hop)
    assert np.all(got[1][:, T:] == 0.0)


def test_inverse_row_strided_input_is_bit_identical():
    """y as a column slice of a wider tensor (row stride above the length) gives the bits of the contiguous call."""
    from golf_amd import functional as GF

    B, F, M, hop, T = 3, 5, 40, 16, 60
    y, a, ge = _inputs(B, F, M, T, 9)
    wide = torch.full((B, T + 37), float("nan"), device="cuda")
    wide[:, 5:5 + T] = dev(y)
    view = wide[:, 5:5 + T]
    assert view.stride(0) == T + 37 and not view.is_contiguous()
    outs = []
    for src in (view, dev(y)):
        yt, at = src.detach().requires_grad_(True), dev(a, True)
        e = GF.ltv_inverse(yt, at, hop)
        (e * dev(ge)).sum().backward()
        outs.append((e.detach(), yt.grad, at.grad))
    assert outs[0][1].shape == (B, T)
    for u, v in zip(*outs):
        assert torch.isfinite(u).all() and torch.equal(u, v)
    _check("inverse strided", [t.cpu().numpy() for t in outs[0]], y, a, ge, hop)


@pytest.mark.parametrize("need_y,need_a", [(True, False), (False, True)])
def test_inverse_one_gradient_alone(need_y, need_a):
    B, F, M, hop, T = 2, 6, 47, 9, 44
    y, a, ge = _inputs(B, F, M, T, 10)
    got = _run(y, a, ge, hop, need_y, need_a)
    assert (got[1] is None) == (not need_y) and (got[2] is None) == (not need_a)
    _check(f"inverse grad y={need_y} a={need_a}", got, y, a, ge, hop)


def test_inverse_rejects_order_65():
    from golf_amd import _lib
    from golf_amd import functional as GF

    with pytest.raises(_lib.GolfError):
        GF.ltv_inverse(torch.zeros(2, 100, device="cuda"), torch.zeros(2, 3, 65, device="cuda"), 50)
