"""The sample-wise LTV all-pole filter from an initial state ``zi`` on every plan, and differentiable through it:
functional.ltv_allpole_ss(zi=..., return_zf=...), ltv_allpole_ss_blocks, ltv_allpole_ss_state(mode=...) and the module
(csrc/lpc_state.hip in front of the unchanged kernels of csrc/lpc_ss.hip / lpc_any.hip).

References: the float64 oracle O.sample_wise_lpc(x, A, zi) for the forward and the final state; for the gradients the float64
autograd recursion of tests/test_lpc_ss_state_host.py (pinned there to the oracle); for the chained blocks the oracle's
zero-state forward and backward over the whole utterance.  Bar: <= 1e-4 relative (max-norm and L2), the project's bar for
these inputs (smooth reflection-coefficient tracks, ``scale`` 0.5, 0.25 for M >= 39: tests/test_gpu_lpc_ss_anyshape.py); an
fp32 emulation of the head correction followed by the sequential recursion sits at 3e-6 or below against the oracle.
zi ~ N(0, 0.3); the cases marked ``zero`` hold an exact 0 in gain[0, 0] (the gain is never divided out of the head)."""
import warnings

import numpy as np
import pytest
import torch

from conftest import rel_err
from test_lpc_ss_state_host import torch_ref_grads

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


_cases, _grads = {}, {}


def case(B, F, M, hop, Tx=None, length=None, zero=False):
    """Inputs, zi, both cotangents and the oracle's forward and final state of one shape (computed once, never modified)."""
    key = (B, F, M, hop, Tx, length, zero)
    if key not in _cases:
        from oracle import golf_oracle as O

        ex, gain, a = smooth_case(B, F, M, hop, Tx=Tx, seed=B * 100 + F, scale=0.25 if M >= 39 else 0.5)
        if zero:
            gain[0, 0] = 0.0
        T = min(ex.shape[1], (F - 1) * hop + 1, length or 10 ** 9)
        rng = np.random.default_rng(7)
        zi = rng.normal(0, 0.3, (B, M)).astype(np.float32)
        gy = rng.normal(0, 1, (B, T)).astype(np.float32)
        gzf = rng.normal(0, 1, (B, M)).astype(np.float32)
        x = ex[:, :T].astype(np.float64) * O.linear_upsample(gain, hop)[:, :T]
        y = O.sample_wise_lpc(x, O.linear_upsample(a, hop)[:, :T], zi)
        zf = np.concatenate([y[:, ::-1][:, :M], zi[:, :max(M - T, 0)].astype(np.float64)], 1)
        for v in (ex, gain, a, zi, gy, gzf, y, zf):
            v.setflags(write=False)
        _cases[key] = dict(ex=ex, gain=gain, a=a, zi=zi, gy=gy, gzf=gzf, T=T, y=y, zf=zf, hop=hop, length=length, key=key)
    return _cases[key]


def ref_grads(c):
    """float64 autograd gradients (g_ex, g_gain, g_a, g_zi) of sum(y gy) + sum(zf gzf), once per case."""
    if c["key"] not in _grads:
        out = torch_ref_grads(c["ex"], c["gain"], c["a"], c["hop"], c["zi"], c["gy"], c["gzf"], c["length"])
        np.testing.assert_allclose(out[0], c["y"], rtol=0, atol=1e-10)   # the two references agree on the forward
        _grads[c["key"]] = out[2:]
    return _grads[c["key"]]


def run(c, mode=None, grads=(True, True, True, True)):
    """(y, zf, g_ex, g_gain, g_a, g_zi) of the product for the case's cotangents."""
    from golf_amd import functional as GF

    leaves = [dev(c[k]).requires_grad_(g) for k, g in zip(("ex", "gain", "a", "zi"), grads)]
    y, zf = GF.ltv_allpole_ss(*leaves[:3], c["hop"], mode=mode, length=c["length"], zi=leaves[3], return_zf=True)
    if any(grads):
        ((y * dev(c["gy"])).sum() + (zf * dev(c["gzf"])).sum()).backward()
    torch.cuda.synchronize()
    return (y.detach(), zf.detach()) + tuple(v.grad for v in leaves)


@pytest.mark.parametrize("B,F,M,hop,Tx,length,mode,zero", [
    (2, 9, 22, 240, None, None, None, True),          # on the ring grid: every plan serves zi
    (2, 9, 22, 240, None, None, "chunked", True),
    (2, 9, 22, 240, None, None, "flat-scan", True),
    (2, 9, 22, 240, None, None, "serial", True),
    (2, 9, 22, 100, None, None, None, False),         # off the grid
    (2, 4, 64, 7, None, None, None, False),           # T = 22 < M, the head spans ten frames
    (1, 1, 4, 7, None, None, None, False),            # F = 1: one sample
    (2, 200, 5, 1, None, None, None, False),          # hop 1
    (3, 10, 22, 100, 777, None, None, False),         # ends inside a frame
    (2, 9, 22, 240, None, 720, None, False),          # a length cut
    (9, 4, 12, 50, None, None, None, False),          # a batch that does not fill a workgroup
])
def test_forward_and_final_state_vs_oracle(B, F, M, hop, Tx, length, mode, zero):
    from golf_amd import functional as GF

    c = case(B, F, M, hop, Tx, length, zero)
    with torch.no_grad():
        y, zf = GF.ltv_allpole_ss(dev(c["ex"]), dev(c["gain"]), dev(c["a"]), hop, mode=mode, length=length, zi=dev(c["zi"]),
                                  return_zf=True)
    torch.cuda.synchronize()
    assert y.shape == (B, c["T"]) and zf.shape == (B, M)
    check(y.cpu().numpy(), c["y"], "y")
    check(zf.cpu().numpy(), c["zf"], "zf")


@pytest.mark.parametrize("B,F,M,hop,Tx,mode,zero", [
    (2, 5, 22, 240, None, "chunked", True),
    (2, 5, 22, 240, None, "serial", True),
    (2, 9, 22, 100, None, None, False),
    (2, 4, 64, 7, None, None, False),
    (1, 1, 4, 7, None, None, False),
    (3, 10, 22, 100, 1200, None, False),              # excitation longer than the output: the tail of g_ex is exactly 0
])
def test_gradients_vs_float64_autograd(B, F, M, hop, Tx, mode, zero):
    c = case(B, F, M, hop, Tx, None, zero)
    y, zf, g_ex, g_gain, g_a, g_zi = run(c, mode)
    r_ex, r_gain, r_a, r_zi = ref_grads(c)
    assert g_ex.shape == c["ex"].shape and g_gain.shape == c["gain"].shape and g_a.shape == c["a"].shape
    assert g_zi.shape == c["zi"].shape
    check(y.cpu().numpy(), c["y"], "y")
    check(zf.cpu().numpy(), c["zf"], "zf")
    check(g_ex.cpu().numpy(), r_ex, "g_ex")
    check(g_gain.cpu().numpy(), r_gain, "g_gain")
    check(g_a.cpu().numpy(), r_a, "g_a")
    check(g_zi.cpu().numpy(), r_zi, "g_zi")
    if c["ex"].shape[1] > c["T"]:
        assert torch.equal(g_ex[:, c["T"]:], torch.zeros_like(g_ex[:, c["T"]:]))


def test_partial_grads():
    c = case(2, 9, 22, 100)
    full = run(c)[2:]
    sets = [tuple(i == only for i in range(4)) for only in range(4)] + [(True, False, False, True), (False, True, True, False)]
    for grads in sets:
        got = run(c, grads=grads)[2:]
        for i in range(4):
            if grads[i]:
                assert torch.equal(got[i], full[i]), (grads, i)
            else:
                assert got[i] is None, (grads, i)


@pytest.mark.parametrize("B,F,M,hop,n", [(3, 13, 22, 240, 4), (2, 13, 22, 100, 5)])
def test_chained_blocks_vs_one_shot_oracle(B, F, M, hop, n):
    """Blocks chained through zf -> zi from zeros ARE the zero-state filter of the whole: y and the gradients w.r.t. ex, gain
    and a against the oracle's one-shot forward and backward.  The gradients reach a block only through the states that
    follow it, so this holds the backward through zf and zi to the bar with no new oracle."""
    from golf_amd import functional as GF
    from oracle import golf_oracle as O

    ex, gain, a = smooth_case(B, F, M, hop, seed=B * 100 + F)
    T = (F - 1) * hop + 1
    gy = np.random.default_rng(1).normal(0, 1, (B, T)).astype(np.float32)
    r_y = O.ltv_allpole_ss_forward(ex, gain, a, hop)
    r_ex, r_gain, r_a = O.ltv_allpole_ss_backward(gy, ex, gain, a, hop)
    out = {}
    for detach in (False, True):
        leaves = [dev(v).requires_grad_(True) for v in (ex, gain, a)]
        y, zf = GF.ltv_allpole_ss_blocks(*leaves, hop, n, detach_state=detach)
        (y * dev(gy)).sum().backward()
        torch.cuda.synchronize()
        out[detach] = (y.detach(), zf.detach()) + tuple(v.grad for v in leaves)
    y, zf, g_ex, g_gain, g_a = out[False]
    assert y.shape == (B, T)
    check(y.cpu().numpy(), r_y, "y")
    check(zf.cpu().numpy(), r_y[:, ::-1][:, :M], "zf")
    check(g_ex.cpu().numpy(), r_ex, "g_ex")
    check(g_gain.cpu().numpy(), r_gain, "g_gain")
    check(g_a.cpu().numpy(), r_a, "g_a")
    # truncated BPTT: the same forward bits, and a first block that no longer hears from the blocks behind it
    first = n * hop
    assert torch.equal(out[True][0], y)
    assert not torch.equal(out[True][2][:, :first], g_ex[:, :first])
    assert torch.equal(out[True][2][:, -hop:], g_ex[:, -hop:])   # (the last block has nothing behind it: unchanged)


def test_zero_state_return_zf_is_the_plain_call():
    from golf_amd import functional as GF

    c = case(2, 9, 22, 240, None, None, True)
    args = (dev(c["ex"]), dev(c["gain"]), dev(c["a"]), 240)
    with torch.no_grad():
        plain = GF.ltv_allpole_ss(*args)
        y, zf = GF.ltv_allpole_ss(*args, zi=None, return_zf=True)
    assert torch.equal(y, plain)
    assert torch.equal(zf, plain.flip(1)[:, :22])


def test_backward_is_reproducible():
    c = case(2, 5, 22, 240, None, None, True)
    first, second = run(c, "chunked"), run(c, "chunked")
    for u, v in zip(first, second):
        assert torch.equal(u, v)
    c = case(2, 4, 64, 7)
    first, second = run(c), run(c)
    for u, v in zip(first, second):
        assert torch.equal(u, v)


def test_strided_rows_scalar_path():
    """ex as a view that starts 5 floats into a wider buffer: no 16-byte alignment, the kernels' scalar path."""
    from golf_amd import functional as GF

    c = case(2, 9, 22, 100)
    B, T = c["ex"].shape
    wide = torch.zeros(B, T + 37, device="cuda")
    wide[:, 5:5 + T] = dev(c["ex"])
    wide.requires_grad_(True)
    gain_t, a_t, zi_t = (dev(c[k]).requires_grad_(True) for k in ("gain", "a", "zi"))
    y, zf = GF.ltv_allpole_ss(wide[:, 5:5 + T], gain_t, a_t, 100, zi=zi_t, return_zf=True)
    ((y * dev(c["gy"])).sum() + (zf * dev(c["gzf"])).sum()).backward()
    torch.cuda.synchronize()
    r_ex, r_gain, r_a, r_zi = ref_grads(c)
    check(y.detach().cpu().numpy(), c["y"], "y")
    check(wide.grad[:, 5:5 + T].cpu().numpy(), r_ex, "g_ex")
    assert not wide.grad[:, :5].any() and not wide.grad[:, 5 + T:].any()
    check(gain_t.grad.cpu().numpy(), r_gain, "g_gain")
    check(a_t.grad.cpu().numpy(), r_a, "g_a")
    check(zi_t.grad.cpu().numpy(), r_zi, "g_zi")


def test_module_state_and_errors():
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import LTVMinimumPhaseFilterPrecise

    B, F, M, hop = 2, 9, 22, 240
    c = case(B, F, M, hop, None, None, True)
    filt = LTVMinimumPhaseFilterPrecise(lpc_order=M).cuda()
    ex_t, gain_t, a_t, zi_t = (dev(c[k]).requires_grad_(True) for k in ("ex", "gain", "a", "zi"))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        y, zf = filt(AudioTensor(ex_t), AudioTensor(gain_t, hop), AudioTensor(a_t, hop), zi=zi_t, return_zf=True)
        assert isinstance(y, AudioTensor) and isinstance(zf, torch.Tensor) and zf.shape == (B, M)
        ((y.as_tensor() * dev(c["gy"])).sum() + (zf * dev(c["gzf"])).sum()).backward()
        torch.cuda.synchronize()
    r_ex, r_gain, r_a, r_zi = ref_grads(c)
    check(y.as_tensor().detach().cpu().numpy(), c["y"], "y")
    check(zf.detach().cpu().numpy(), c["zf"], "zf")
    for got, ref, what in ((ex_t, r_ex, "g_ex"), (gain_t, r_gain, "g_gain"), (a_t, r_a, "g_a"), (zi_t, r_zi, "g_zi")):
        check(got.grad.cpu().numpy(), ref, what)
    plain = filt(AudioTensor(dev(c["ex"])), AudioTensor(dev(c["gain"]), hop), AudioTensor(dev(c["a"]), hop))
    assert isinstance(plain, AudioTensor)

    # the carried-state entry on a fast plan: y and the state it leaves behind
    state = dev(c["zi"])
    ys = GF.ltv_allpole_ss_state(dev(c["ex"]), dev(c["gain"]), dev(c["a"]), hop, state, mode="chunked")
    torch.cuda.synchronize()
    check(ys.cpu().numpy(), c["y"], "state y")
    assert torch.equal(state, ys.flip(1)[:, :M])
    check(state.cpu().numpy(), c["zf"], "state")

    for bad in (torch.zeros(B, M + 1, device="cuda"), torch.zeros(B + 1, M, device="cuda"), torch.zeros(B * M, device="cuda"),
                torch.zeros(B, M), torch.zeros(B, M, device="cuda", dtype=torch.float64)):
        with pytest.raises(GolfError):
            GF.ltv_allpole_ss(dev(c["ex"]), dev(c["gain"]), dev(c["a"]), hop, zi=bad)
