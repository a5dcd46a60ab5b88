"""CPU: the arithmetic behind the sample-wise LPC filter's differentiable initial state (csrc/lpc_state.hip,
functional.ltv_allpole_ss(zi=..., return_zf=...), functional.ltv_allpole_ss_blocks), without a GPU.

* ``torch_ref`` -- a float64 torch recursion with autograd, initial state ``zi`` and final state ``zf`` included -- is the
  gradient reference of tests/test_gpu_lpc_ss_state_grad.py.  It is pinned here to the oracle: forward == O.sample_wise_lpc(x,
  A, zi) to 1e-12, and with zi = 0 its gradients == O.ltv_allpole_ss_backward.
* ``identity_np`` states in numpy what the product computes: a filter from ``zi`` is the ZERO-STATE filter of an excitation
  whose first min(M, T) samples carry a correction (gain applied, never divided out), and its gradients follow from the
  zero-state backward.  It equals the reference to 1e-10 for the forward, zf and all four gradients, T < M and a ``length``
  cut included.
* The block boundaries of ltv_allpole_ss_blocks are pure host arithmetic: with the kernel call replaced by ``torch_ref`` the
  chain reproduces the one-shot recursion to 1e-12."""
import numpy as np
import pytest
import torch

from oracle import golf_oracle as O


def up_t(z: torch.Tensor, hop: int) -> torch.Tensor:
    """oracle.linear_upsample along dim 1 on a float64 torch tensor (differentiable)."""
    F = z.shape[1]
    if hop == 1 or F == 1:
        return z
    n = torch.arange((F - 1) * hop + 1)
    f = torch.clamp(n // hop, max=F - 2)
    w = ((n - f * hop).double() / hop).reshape((1, -1) + (1,) * (z.dim() - 2))
    return z[:, f] * (1.0 - w) + z[:, f + 1] * w


def torch_ref(ex, gain, a, hop, zi=None, length=None):
    """float64 recursion y[t] = ex[t] up(gain)[t] - sum_i up(a)[t,i] y[t-1-i] from y[-1-j] = zi[j]; returns (y, zf) with
    zf[j] = y[T-1-j] (the history list carries zi, so T < M shifts the old state in by itself).  Differentiable."""
    B, F, M = a.shape
    G, A = up_t(gain, hop), up_t(a, hop)
    T = min(ex.shape[1], G.shape[1])
    if length is not None:
        T = min(T, int(length))
    x = ex[:, :T] * G[:, :T]
    past = zi if zi is not None else x.new_zeros(B, M)   # past[:, i] = y[t-1-i]
    ys = []
    for t in range(T):
        yt = x[:, t] - (A[:, t] * past).sum(1)
        ys.append(yt)
        past = torch.cat([yt[:, None], past[:, :-1]], 1)
    y = torch.stack(ys, 1) if ys else x
    return y, past


def torch_ref_grads(ex, gain, a, hop, zi, gy, gzf, length=None):
    """(y, zf, g_ex, g_gain, g_a, g_zi) of torch_ref as float64 numpy arrays, for cotangents gy on y and gzf on zf."""
    leaves = [torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for v in (ex, gain, a, zi)]
    y, zf = torch_ref(*leaves[:3], hop, leaves[3], length)
    loss = (y * torch.tensor(np.asarray(gy, dtype=np.float64))).sum() + (zf * torch.tensor(np.asarray(gzf, dtype=np.float64))).sum()
    loss.backward()
    return (y.detach().numpy(), zf.detach().numpy()) + tuple(v.grad.numpy() for v in leaves)


def identity_np(ex, gain, a, hop, zi, gy, gzf, length=None):
    """The identity the kernels implement, in float64 numpy on the oracle's ZERO-STATE forward and backward."""
    ex, gain, a, zi = (np.asarray(v, dtype=np.float64) for v in (ex, gain, a, zi))
    B, F, M = a.shape
    G, A = O.linear_upsample(gain, hop), O.linear_upsample(a, hop)
    T = min(ex.shape[1], G.shape[1])
    if length is not None:
        T = min(T, int(length))
    G, A = G[:, :T], A[:, :T]
    H = min(M, T)
    xh = ex[:, :T] * G
    for t in range(H):
        for i in range(t, M):
            xh[:, t] -= A[:, t, i] * zi[:, i - t]
    ones = np.ones((B, F))
    y = O.ltv_allpole_ss_forward(xh, ones, a, hop)
    zf = np.concatenate([y[:, ::-1][:, :M], zi[:, :max(M - T, 0)]], 1)
    # backward: the cotangent of zf lands on y's last samples (and, for T < M, on zi directly)
    gyt = np.array(gy, dtype=np.float64)
    g_zi = np.zeros((B, M))
    for j in range(M):
        if j < T:
            gyt[:, T - 1 - j] += gzf[:, j]
        else:
            g_zi[:, j - T] += gzf[:, j]
    q, _, g_a = O.ltv_allpole_ss_backward(gyt, xh, ones, a, hop)
    g_ex = np.zeros_like(ex)
    g_ex[:, :T] = q * G
    g_gain = O._upsample_adjoint(q * ex[:, :T], hop, F)
    gAh = np.zeros((B, T, M))
    for t in range(H):
        for i in range(t, M):
            gAh[:, t, i] = -q[:, t] * zi[:, i - t]
        for j in range(M - t):
            g_zi[:, j] -= q[:, t] * A[:, t, t + j]
    g_a = g_a + O._upsample_adjoint(gAh, hop, F)
    return y, zf, g_ex, g_gain, g_a, g_zi


def random_case(B, F, M, hop, Tx, seed=0):
    rng = np.random.default_rng(seed)
    a = O.rc2lpc(np.tanh(rng.normal(0, 0.5, (B, 1, M)) + np.cumsum(rng.normal(0, 0.02, (B, F, M)), 1)))
    gain = np.exp(-1 + np.cumsum(rng.normal(0, 0.05, (B, F)), 1))
    gain[0, 0] = 0.0
    ex = rng.normal(0, 1, (B, Tx))
    zi = rng.normal(0, 0.3, (B, M))
    return ex, gain, a, zi, rng


SHAPES = [(3, 5, 6, 8, 40, None), (2, 3, 7, 4, 3, None), (2, 6, 6, 8, 100, 24)]   # T < M; a length cut


@pytest.mark.parametrize("B,F,M,hop,Tx,length", SHAPES)
def test_torch_ref_forward_equals_oracle(B, F, M, hop, Tx, length):
    ex, gain, a, zi, _ = random_case(B, F, M, hop, Tx)
    y, zf = torch_ref(*(torch.tensor(v) for v in (ex, gain, a)), hop, torch.tensor(zi), length)
    T = y.shape[1]
    assert T == min(Tx, (F - 1) * hop + 1, length or 10 ** 9)
    x = ex[:, :T] * O.linear_upsample(gain, hop)[:, :T]
    ref = O.sample_wise_lpc(x, O.linear_upsample(a, hop)[:, :T], zi)
    np.testing.assert_allclose(y.numpy(), ref, rtol=0, atol=1e-12)
    ref_zf = np.concatenate([ref[:, ::-1][:, :M], zi[:, :max(M - T, 0)]], 1)
    np.testing.assert_allclose(zf.numpy(), ref_zf, rtol=0, atol=1e-12)


def test_torch_ref_zero_state_gradients_equal_oracle():
    B, F, M, hop, Tx = 3, 5, 6, 8, 40
    ex, gain, a, _, rng = random_case(B, F, M, hop, Tx)
    T = min(Tx, (F - 1) * hop + 1)
    gy = rng.normal(0, 1, (B, T))
    got = torch_ref_grads(ex, gain, a, hop, np.zeros((B, M)), gy, np.zeros((B, M)))
    np.testing.assert_allclose(got[0], O.ltv_allpole_ss_forward(ex, gain, a, hop), rtol=0, atol=1e-12)
    for g, r in zip(got[2:5], O.ltv_allpole_ss_backward(gy, ex, gain, a, hop)):
        np.testing.assert_allclose(g, r, rtol=0, atol=1e-12)


@pytest.mark.parametrize("B,F,M,hop,Tx,length", SHAPES)
def test_identity_equals_reference(B, F, M, hop, Tx, length):
    ex, gain, a, zi, rng = random_case(B, F, M, hop, Tx, seed=1)
    T = min(Tx, (F - 1) * hop + 1, length or 10 ** 9)
    gy, gzf = rng.normal(0, 1, (B, T)), rng.normal(0, 1, (B, M))
    ref = torch_ref_grads(ex, gain, a, hop, zi, gy, gzf, length)
    got = identity_np(ex, gain, a, hop, zi, gy, gzf, length)
    for name, g, r in zip(("y", "zf", "g_ex", "g_gain", "g_a", "g_zi"), got, ref):
        assert g.shape == r.shape, name
        np.testing.assert_allclose(g, r, rtol=0, atol=1e-10, err_msg=name)


def test_block_bounds():
    from golf_amd.functional import ss_block_bounds

    assert ss_block_bounds(41, 6, 8, 2) == [(0, 2, 0, 16), (2, 4, 16, 32), (4, 5, 32, 41)]
    assert ss_block_bounds(41, 6, 8, 5) == [(0, 5, 0, 41)]
    assert ss_block_bounds(41, 6, 8, 9) == [(0, 5, 0, 41)]
    assert ss_block_bounds(20, 6, 8, 2) == [(0, 2, 0, 16), (2, 4, 16, 20)]      # the utterance ends inside the second block
    assert ss_block_bounds(16, 6, 8, 2) == [(0, 2, 0, 16)]                      # ... exactly at a block boundary
    assert ss_block_bounds(1, 1, 7, 4) == [(0, 0, 0, 1)]
    assert ss_block_bounds(4, 4, 1, 1) == [(0, 1, 0, 1), (1, 2, 1, 2), (2, 3, 2, 4)]


@pytest.mark.parametrize("B,F,M,hop,Tx,length,n", [
    (2, 6, 6, 8, 41, None, 2),     # blocks shorter and longer than M, the last one with the final sample
    (2, 6, 6, 8, 100, 24, 1),      # a length cut: the chain stops with the block that holds sample 23
    (2, 7, 9, 4, 19, None, 1),     # every block shorter than M: the state shifts through several blocks
    (1, 1, 4, 7, 5, None, 3),      # F = 1
    (2, 5, 3, 1, 5, None, 2),      # hop 1
])
def test_blocks_chain_equals_one_shot(monkeypatch, B, F, M, hop, Tx, length, n):
    from golf_amd import functional as GF

    calls = []

    def fake(ex, gain, a, hop, zi=None, return_zf=False, **kw):
        assert return_zf and not kw
        calls.append((ex.shape[1], a.shape[1]))
        return torch_ref(ex, gain, a, hop, zi)

    monkeypatch.setattr(GF, "ltv_allpole_ss", fake)
    ex, gain, a, zi, rng = random_case(B, F, M, hop, Tx, seed=2)
    for z in (None, zi):
        leaves = [torch.tensor(v, requires_grad=True) for v in (ex, gain, a)]
        zt = None if z is None else torch.tensor(z, requires_grad=True)
        y, zf = GF.ltv_allpole_ss_blocks(*leaves, hop, n, zi=zt, length=length)
        ry, rzf = torch_ref(*(torch.tensor(v) for v in (ex, gain, a)), hop, None if z is None else torch.tensor(z), length)
        assert y.shape == ry.shape and zf.shape == rzf.shape
        np.testing.assert_allclose(y.detach().numpy(), ry.numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(zf.detach().numpy(), rzf.numpy(), rtol=0, atol=1e-12)
    T = ry.shape[1]
    assert len(calls) == 2 * len(GF.ss_block_bounds(T, F, hop, n))
    # the gradient reaches the first block through the chain of states, and stops at the boundary with detach_state
    if len(calls) > 2:
        first = GF.ss_block_bounds(T, F, hop, n)[0][3]
        grads = []
        for detach in (False, True):
            x = torch.tensor(ex, requires_grad=True)
            y, _ = GF.ltv_allpole_ss_blocks(x, torch.tensor(gain), torch.tensor(a), hop, n, length=length, detach_state=detach)
            y[:, first:].sum().backward()
            grads.append(x.grad[:, :first].abs().max().item())
        assert grads[0] > 0 and grads[1] == 0
