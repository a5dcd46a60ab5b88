"""The frame-wise LTI all-pole + OLA filter at shapes OFF the ring grid (order 39 .. 64, a hop below the ring width the order
needs, or -- for the backward -- a window that is no multiple of the ring width): forward and all three gradients of the
wave-per-frame kernels (csrc/lpc_ff_any.hip) through LTVMinimumPhaseFilter against the float64 oracle.  Bars as in
tests/test_gpu_lpc_ff.py: forward <= 1e-4, each gradient <= 2e-4, relative max-norm and L2.

Inputs: ``smooth_case`` of tests/test_gpu_lpc_ss_anyshape.py with seed B*100 + F, a Hann window, the cotangent
default_rng(1).normal(0, 1, y.shape).  The base logits of the reflection coefficients have standard deviation ``scale``: 0.25
for the high orders (at 0.5 and M = 64 a numpy fp32 emulation of the plain algorithm -- sequential per-frame recursion, fp32
correlation sums, fp32 overlap-add -- is itself at 1e-4 with |y| ~ 44); with the scales below that emulation stays at or
under 2.3e-6 on y, g_ex and g_a for the first thirteen shapes, more than 40 x inside the bars."""
import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL_Y, TOL_G = 1e-4, 2e-4

#  B   F   M  hop    W    Tx  centred scale
SHAPES = [
    (2, 6, 39, 240, 960, None, True, 0.25),     # first order past the grid at the recipe shape
    (2, 6, 64, 240, 960, None, True, 0.25),     # largest order
    (2, 5, 64, 128, 512, None, True, 0.25),     # largest order, W = 4*hop
    (2, 8, 48, 96, 250, None, True, 0.25),      # W not a multiple of hop, 4 or 64
    (2, 5, 40, 441, 1024, None, True, 0.25),    # odd hop
    (2, 9, 22, 16, 64, None, True, 0.5),        # hop below the ring width of the order
    (3, 12, 5, 4, 8, None, True, 0.5),          # hop < 8, W = 2*hop
    (1, 40, 3, 2, 8, None, True, 0.5),          # hop 2, many frames per sample
    (1, 10, 30, 30, 100, None, True, 0.25),     # hop = M
    (2, 7, 22, 240, 1000, None, True, 0.5),     # ring forward, new backward (1000 % 24 != 0)
    (2, 7, 26, 120, 300, None, False, 0.25),    # centred=False, 300 % 32 != 0
    (3, 10, 48, 100, 400, 777, True, 0.25),     # excitation ends inside a frame
    (9, 4, 45, 50, 128, None, True, 0.25),      # batch that fills no tile
    (1, 3, 64, 32, 64, None, True, 0.25),       # W = 2*hop = M: frame no longer than the filter
    (2, 3, 39, 40, 80, 41, True, 0.25),         # shortest utterance the reference accepts
]
REPRO = (3, 10, 48, 100, 400, 777, True, 0.25)


def dev(x):
    return torch.as_tensor(np.array(x, dtype=np.float32)).cuda()   # (a copy: the shared cases are read-only)


def check(x, ref, what, tol):
    emax, el2 = rel_err(x, ref)
    print(f"{what}: rel-max {emax:.3e} rel-l2 {el2:.3e}")
    assert np.isfinite(x).all(), what
    assert emax <= tol and el2 <= tol, (what, emax, el2)


_cases = {}


def case(B, F, M, hop, W, Tx, centred, scale):
    """Inputs, cotangent and the oracle's forward and gradients of one shape (computed once, never modified)."""
    key = (B, F, M, hop, W, Tx, centred, scale)
    if key not in _cases:
        from oracle import golf_oracle as O
        from test_gpu_lpc_ss_anyshape import smooth_case

        ex, gain, a = smooth_case(B, F, M, hop, Tx=Tx, seed=B * 100 + F, scale=scale)
        win = torch.hann_window(W).double().numpy()
        ref, _ = O.lti_frames_ola_forward(ex, gain, a, hop, win, centred=centred)
        gy = np.random.default_rng(1).normal(0, 1, ref.shape).astype(np.float32)
        refs = (ref,) + tuple(O.lti_frames_ola_backward(gy, ex, gain, a, hop, win, centred=centred))
        for v in (ex, gain, a, gy) + refs:
            v.setflags(write=False)
        _cases[key] = (ex, gain, a, gy, refs)
    return _cases[key]


def leaves(ex, gain, a, grads=(True, True, True)):
    return tuple(dev(v).requires_grad_(g) for v, g in zip((ex, gain, a), grads))


def run(ex_t, gain_t, a_t, gy_t, hop, W, centred, x_in=None):
    """Forward and backward through the module, as tests/test_gpu_lpc_ff.py::run_module_grad does.  ``x_in``: the tensor
    handed to the module as the excitation when it is a view of the leaf ``ex_t``."""
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import LTVMinimumPhaseFilter

    m = LTVMinimumPhaseFilter(window="hanning", window_length=W, centred=centred, lpc_order=a_t.shape[-1]).cuda()
    y = m(AudioTensor(ex_t if x_in is None else x_in), AudioTensor(gain_t, hop), AudioTensor(a_t, hop))
    assert y.hop_length == 1
    y = y.as_tensor()
    (y * gy_t).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), ex_t.grad, gain_t.grad, a_t.grad


@pytest.mark.parametrize("B,F,M,hop,W,Tx,centred,scale", SHAPES)
def test_fwd_bwd_vs_oracle(B, F, M, hop, W, Tx, centred, scale):
    ex, gain, a, gy, (r_y, r_ex, r_gain, r_a) = case(B, F, M, hop, W, Tx, centred, scale)
    y, g_ex, g_gain, g_a = run(*leaves(ex, gain, a), dev(gy), hop, W, centred)
    assert y.shape == r_y.shape and g_ex.shape == ex.shape and g_gain.shape == gain.shape and g_a.shape == a.shape
    check(y.cpu().numpy(), r_y, "y", TOL_Y)
    check(g_ex.cpu().numpy(), r_ex, "g_ex", TOL_G)
    check(g_gain.cpu().numpy(), r_gain, "g_gain", TOL_G)
    check(g_a.cpu().numpy(), r_a, "g_a", TOL_G)


def test_partial_grads():
    """requires_grad on one input at a time gives the bits of the full backward."""
    B, F, M, hop, W, Tx, centred, scale = SHAPES[0]
    ex, gain, a, gy, _ = case(*SHAPES[0])
    full = run(*leaves(ex, gain, a), dev(gy), hop, W, centred)[1:]
    for only in range(3):
        grads = run(*leaves(ex, gain, a, tuple(i == only for i in range(3))), dev(gy), hop, W, centred)[1:]
        for i in range(3):
            if i == only:
                assert torch.equal(grads[i], full[i])
            else:
                assert grads[i] is None


def test_backward_is_reproducible():
    B, F, M, hop, W, Tx, centred, scale = REPRO
    ex, gain, a, gy, _ = case(*REPRO)
    first = run(*leaves(ex, gain, a), dev(gy), hop, W, centred)
    second = run(*leaves(ex, gain, a), dev(gy), hop, W, centred)
    for u, v in zip(first, second):
        assert torch.equal(u, v)


def test_strided_excitation():
    """A non-contiguous excitation (a column slice of a wider tensor) gives the bits of the contiguous one."""
    B, F, M, hop, W, Tx, centred, scale = SHAPES[3]
    ex, gain, a, gy, _ = case(*SHAPES[3])
    want = run(*leaves(ex, gain, a), dev(gy), hop, W, centred)
    T = ex.shape[1]
    wide = torch.zeros(B, T + 37, device="cuda")
    wide[:, 5:5 + T] = dev(ex)
    wide.requires_grad_(True)
    view = wide[:, 5:5 + T]
    assert not view.is_contiguous()
    _, gain_t, a_t = leaves(ex, gain, a)
    y, g_wide, g_gain, g_a = run(wide, gain_t, a_t, dev(gy), hop, W, centred, x_in=view)
    assert torch.equal(y, want[0])
    assert torch.equal(g_wide[:, 5:5 + T], want[1])
    assert not g_wide[:, :5].any() and not g_wide[:, 5 + T:].any()
    assert torch.equal(g_gain, want[2]) and torch.equal(g_a, want[3])


def test_order_limit():
    """M = 65 is refused, and the message names the limit."""
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError
    from test_gpu_lpc_ss_anyshape import smooth_case

    ex, gain, a = smooth_case(1, 4, 65, 240, seed=104, scale=0.25)
    with pytest.raises(GolfError, match="M <= 64"):
        GF.lti_frames_ola(dev(ex), dev(gain), dev(a), torch.hann_window(960, device="cuda"), 240)
