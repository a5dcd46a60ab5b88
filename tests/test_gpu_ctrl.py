"""GPU parity of the fused LPC control transform (golf_rc2lpc_{fwd,bwd}_f32; reference rc2lpc, models/utils.py:581-593,
as used by models/filters.py:91-97): the reference's own output (golden g1), the PyTorch restatement in float64 at the
BASELINE shape, gradients against autograd of that restatement, and the stability property of the step-up."""
import numpy as np
import pytest
import torch

import parity
from conftest import rel_err

pytestmark = pytest.mark.gpu


def test_golden_g1(golden):
    from golf_amd import functional as GF

    g = golden("g1_rc2lpc")
    for rc_key, out_key in (("rc", "lpc"), ("rc1", "lpc1")):
        rc = torch.as_tensor(np.asarray(g[rc_key]), dtype=torch.float32).cuda()
        a = GF.rc2lpc(rc).cpu().numpy()
        emax, el2 = rel_err(a, np.asarray(g[out_key]))
        print("g1", rc_key, emax, el2)
        assert emax < 2e-6 and el2 < 2e-6


@pytest.mark.parametrize("B,F,M,max_abs", [(32, 200, 22, 1.0), (3, 7, 1, 1.0), (2, 5, 2, 0.99), (2, 9, 7, 0.9),
                                             (1, 300, 64, 0.95)])
def test_forward_and_backward_vs_torch(B, F, M, max_abs):
    from golf_amd import functional as GF
    from golf_amd.utils import rc2lpc

    gen = torch.Generator().manual_seed(B * 100 + M)
    logits = torch.randn(B, F, M, generator=gen) * 0.7
    gy = torch.randn(B, F, M, generator=gen)
    ref_in = logits.double().requires_grad_(True)
    ref = rc2lpc(torch.tanh(ref_in) * max_abs)
    (ref * gy.double()).sum().backward()
    x = logits.cuda().requires_grad_(True)
    a = GF.rc2lpc_logits(x, max_abs)
    assert a.shape == (B, F, M)
    (a * gy.cuda()).sum().backward()
    emax, el2 = rel_err(a.detach().cpu().numpy(), ref.detach().numpy())
    gmax, gl2 = rel_err(x.grad.cpu().numpy(), ref_in.grad.numpy())
    print(f"rc2lpc B{B} F{F} M{M}: fwd {emax:.2e} {el2:.2e}  grad {gmax:.2e} {gl2:.2e}")
    tol = 2e-5 if M > 32 else 5e-6
    assert emax < tol and el2 < tol and gmax < 10 * tol and gl2 < 10 * tol


def test_module_ctrl_uses_the_fused_kernel_and_matches_cpu_path():
    """The filter's .ctrl transform on GPU tensors (one kernel) equals the same transform on CPU tensors (PyTorch ops),
    values and gradients, and the result is a minimum-phase polynomial (|k| < 1 <=> all roots inside the unit circle)."""
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import LTVMinimumPhaseFilterPrecise

    m = LTVMinimumPhaseFilterPrecise(lpc_order=22, lpc_parameterisation="rc2lpc", max_abs_value=0.99)
    (split, trsfms) = m.ctrl(lambda s_, t_: (s_, t_))((), ())
    assert split[0] == (1, 22)
    gen = torch.Generator().manual_seed(4)
    lg, lo = torch.randn(4, 50, generator=gen) * 0.1, torch.randn(4, 50, 22, generator=gen)
    outs = {}
    for dev in ("cpu", "cuda"):
        l1 = lo.detach().clone().to(dev).requires_grad_(True)
        gain, a = trsfms[0](AudioTensor(lg.to(dev), 240), AudioTensor(l1, 240))
        a.as_tensor().square().sum().backward()
        outs[dev] = (gain.as_tensor().detach().cpu(), a.as_tensor().detach().cpu(), l1.grad.cpu())
        assert a.hop_length == 240
    for what, u, v in zip(("gain", "a", "grad"), outs["cpu"], outs["cuda"]):
        emax, el2 = rel_err(v.numpy(), u.numpy())        # both sides fp32: max-norm relative difference
        print("ctrl cpu vs gpu", what, emax, el2)
        assert emax < 1e-4 and el2 < 1e-4
    poly = np.concatenate([np.ones((4, 50, 1)), outs["cuda"][1].double().numpy()], -1)
    radii = np.abs(np.roots(poly[0, 0]))
    assert radii.max() < 1.0


def test_errors():
    from golf_amd import _lib
    from golf_amd import functional as GF

    with pytest.raises(_lib.GolfError):
        GF.rc2lpc_logits(torch.zeros(2, 3, 65, device="cuda"))   # order above the kernel's limit
    with pytest.raises(_lib.GolfError):
        GF.rc2lpc_logits(torch.zeros(2, 3, 4))                     # CPU tensor: there is no CPU path in the library


@pytest.mark.parametrize("rep", ["coef", "conj", "real"])
@pytest.mark.parametrize("B,F,K", [(32, 200, 11), (2, 9, 1), (3, 17, 13), (1, 40, 32)])
def test_biquad_parameterisations_vs_torch(rep, B, F, K):
    """golf_sos2lpc_{fwd,bwd}_f32 (logits -> K biquads -> direct form, the ISMIR'23 parameterisations) against the
    PyTorch restatement pinned by golden g2, in float64, values and gradients."""
    from golf_amd import functional as GF
    from golf_amd.utils import biquads2lpc, get_logits2biquads

    gen = torch.Generator().manual_seed(K * 10 + len(rep))
    logits = torch.randn(B, F, 2 * K, generator=gen) * 0.8
    gy = torch.randn(B, F, 2 * K, generator=gen)
    ref_in = logits.double().requires_grad_(True)
    ref = biquads2lpc(get_logits2biquads(rep, 0.97)(ref_in.view(B, F, K, 2)))
    (ref * gy.double()).sum().backward()
    x = logits.cuda().requires_grad_(True)
    a = GF.biquad_logits2lpc(x, rep, 0.97)
    assert a.shape == (B, F, 2 * K)
    (a * gy.cuda()).sum().backward()
    emax, el2 = rel_err(a.detach().cpu().numpy(), ref.detach().numpy())
    gmax, gl2 = rel_err(x.grad.cpu().numpy(), ref_in.grad.numpy())
    print(f"sos2lpc {rep} B{B} F{F} K{K}: fwd {emax:.2e} {el2:.2e}  grad {gmax:.2e} {gl2:.2e}")
    tol = 5e-5 if K > 16 else 5e-6          # a degree-64 product in fp32
    assert emax < tol and el2 < tol and gmax < 10 * tol and gl2 < 10 * tol


def test_golden_g2_biquads(golden):
    """The reference's own logits -> biquads -> direct form (g2, default pole radius 0.99) through the fused kernel."""
    from golf_amd import functional as GF

    g = golden("g2_biquads")
    lg = torch.as_tensor(np.asarray(g["logits"]), dtype=torch.float32)
    flat = lg.reshape(*lg.shape[:-2], -1).cuda()
    for rep in ("coef", "conj", "real"):
        a = GF.biquad_logits2lpc(flat, rep, 0.99).cpu().numpy()
        emax, el2 = rel_err(a, np.asarray(g[f"lpc_{rep}"]))
        print("g2", rep, emax, el2)
        assert emax < 5e-6 and el2 < 5e-6


# ----------------------------------------------------------------------------------------------------------------------
# Every branch of the launchers.  B = 3, F = 43: N = 129 frames, two full 64-lane blocks plus one lane in a third.
# Each result is held to the file's global bounds and, frame by frame, to tests/parity.py's per-frame bound.
# ----------------------------------------------------------------------------------------------------------------------
RC_WORST = parity.Worst("rc2lpc")
SOS_WORST = parity.Worst("sos2lpc")
CAP, CAP_COEF = 0.10, 1.0 / 3.0      # largest share of frames that may sit on the loosened per-frame allowance


def _rc_tol(M):
    return 2e-5 if M > 32 else 5e-6


def _sos_tol(K):
    return 5e-5 if K > 16 else 5e-6          # a degree-64 product in fp32


def _run_ctrl(gpu_fn, ref_fn, logits, gy):
    """(values, gradient) of the kernel, of the float64 restatement and of the fp32 restatement on the CPU."""
    x = logits.cuda().requires_grad_(True)
    a = gpu_fn(x)
    assert a.shape == logits.shape
    (a * gy.cuda()).sum().backward()
    got = (a.detach().cpu().numpy(), x.grad.cpu().numpy())
    return got, parity.torch_restatement(ref_fn, logits, gy, torch.float64), \
        parity.torch_restatement(ref_fn, logits, gy, torch.float32)


def _check_ctrl(worst, what, got, r64, r32, tol, cap):
    parity.check_frames(worst, what + " fwd", got[0], r64[0], r32[0], tol, cap)
    parity.check_frames(worst, what + " grad", got[1], r64[1], r32[1], 10 * tol, cap)


def _check_ctrl_global(worst, what, got, r64, tol):
    for g in got:
        assert np.isfinite(g).all(), what
    parity.check_global(worst, what + " fwd", got[0], r64[0], tol)
    parity.check_global(worst, what + " grad", got[1], r64[1], 10 * tol)


# order -> (forward kernel, backward kernel) of golf_rc2lpc_{fwd,bwd}_f32; the forward switches to the LDS kernel above
# order 32, the backward above order 24:
#    8: fwd reg<8>,  bwd reg<8>       9: fwd reg<16>, bwd reg<16>     16: fwd reg<16>, bwd reg<16>
#   17: fwd reg<24>, bwd reg<24>     24: fwd reg<24>, bwd reg<24>     25: fwd reg<32>, bwd LDS
#   32: fwd reg<32>, bwd LDS         33: fwd LDS,     bwd LDS         47, 64: fwd LDS, bwd LDS
@pytest.mark.parametrize("max_abs", [1.0, 0.99])
@pytest.mark.parametrize("M", [8, 9, 16, 17, 24, 25, 32, 33, 47, 64])
def test_rc2lpc_every_kernel_per_frame(M, max_abs):
    from golf_amd import functional as GF
    from golf_amd.utils import rc2lpc

    gen = torch.Generator().manual_seed(1000 + M)
    logits = torch.randn(3, 43, M, generator=gen) * 0.7
    gy = torch.randn(3, 43, M, generator=gen)
    got, r64, r32 = _run_ctrl(lambda x: GF.rc2lpc_logits(x, max_abs), lambda x: rc2lpc(torch.tanh(x) * max_abs), logits, gy)
    _check_ctrl(RC_WORST, f"rc2lpc tanh M{M} max_abs {max_abs}", got, r64, r32, _rc_tol(M), CAP)


# apply_tanh = 0: 1 -> reg<8> / reg<8>, 12 -> reg<16> / reg<16>, 25 -> fwd reg<32>, bwd LDS, 40 -> LDS / LDS
@pytest.mark.parametrize("M", [1, 12, 25, 40])
def test_rc2lpc_without_tanh_per_frame(M):
    from golf_amd import functional as GF
    from golf_amd.utils import rc2lpc

    gen = torch.Generator().manual_seed(2000 + M)
    rc = torch.tanh(torch.randn(3, 43, M, generator=gen) * 0.5) * 0.98
    gy = torch.randn(3, 43, M, generator=gen)
    got, r64, r32 = _run_ctrl(GF.rc2lpc, rc2lpc, rc, gy)
    _check_ctrl(RC_WORST, f"rc2lpc plain M{M}", got, r64, r32, _rc_tol(M), CAP)


@pytest.mark.parametrize("N", [1, 64, 65])
def test_rc2lpc_block_edges(N):
    """One frame, exactly one block, one block plus one lane (order 12: the reg<16> kernels)."""
    from golf_amd import functional as GF
    from golf_amd.utils import rc2lpc

    gen = torch.Generator().manual_seed(3000 + N)
    logits = torch.randn(1, N, 12, generator=gen) * 0.7
    gy = torch.randn(1, N, 12, generator=gen)
    got, r64, r32 = _run_ctrl(lambda x: GF.rc2lpc_logits(x, 0.99), lambda x: rc2lpc(torch.tanh(x) * 0.99), logits, gy)
    _check_ctrl(RC_WORST, f"rc2lpc N{N}", got, r64, r32, _rc_tol(12), CAP)


@pytest.mark.parametrize("max_abs", [1.0, 0.99])
@pytest.mark.parametrize("M", [22, 64])
def test_rc2lpc_saturated_logits(M, max_abs):
    """Reflection coefficients at (max_abs = 1: on) the stability bound: logits N(0, 6^2) with +-30 (tanh rounds to +-1) and
    exact zeros planted.  Frames differ by orders of magnitude here, so only the global metric is applied."""
    from golf_amd import functional as GF
    from golf_amd.utils import rc2lpc

    gen = torch.Generator().manual_seed(4000 + M)
    logits = torch.randn(3, 43, M, generator=gen) * 6
    flat = logits.view(-1)
    where = torch.randperm(flat.numel(), generator=gen)[:60]
    flat[where[:20]], flat[where[20:40]], flat[where[40:]] = 30.0, -30.0, 0.0
    logits[0, 0, 0], logits[1, 5, M - 1], logits[2, 42, :] = 30.0, -30.0, 0.0
    gy = torch.randn(3, 43, M, generator=gen)
    got, r64, _ = _run_ctrl(lambda x: GF.rc2lpc_logits(x, max_abs), lambda x: rc2lpc(torch.tanh(x) * max_abs), logits, gy)
    _check_ctrl_global(RC_WORST, f"rc2lpc saturated M{M} max_abs {max_abs}", got, r64, _rc_tol(M))


def _sos_fns(rep, rho=0.97):
    from golf_amd import functional as GF
    from golf_amd.utils import biquads2lpc, get_logits2biquads

    to_sos = get_logits2biquads(rep, rho)
    return (lambda x: GF.biquad_logits2lpc(x, rep, rho),
            lambda x: biquads2lpc(to_sos(x.view(*x.shape[:-1], x.shape[-1] // 2, 2))))


@pytest.mark.parametrize("rep", ["coef", "conj", "real"])
@pytest.mark.parametrize("K", [1, 2, 8, 16, 17, 31, 32])
def test_sos2lpc_section_counts_per_frame(rep, K):
    """K = 1 .. 32 sections, every representation, global and per-frame bounds.  "coef" at K = 32 has frames whose product
    grows to 1e11 before it cancels to |a| ~ 1 (condition 6e10); the kernels form the product in double."""
    gen = torch.Generator().manual_seed(5000 + 10 * K + len(rep))
    logits = torch.randn(3, 43, 2 * K, generator=gen) * 0.8
    gy = torch.randn(3, 43, 2 * K, generator=gen)
    got, r64, r32 = _run_ctrl(*_sos_fns(rep), logits, gy)
    _check_ctrl(SOS_WORST, f"sos2lpc {rep} K{K}", got, r64, r32, _sos_tol(K), CAP_COEF if rep == "coef" else CAP)


@pytest.mark.parametrize("K", [2, 13])
def test_sos2lpc_coef_zero_first_logit(K):
    """"coef" has a2 depend on |a1|: at a first-of-pair logit of exactly 0.0 the reference's abs has gradient 0, and so has
    the kernel's sign term."""
    gen = torch.Generator().manual_seed(6000 + K)
    logits = torch.randn(3, 43, 2 * K, generator=gen) * 0.8
    pairs = logits.view(3, 43, K, 2)
    pairs[:, ::3, 0, 0] = 0.0                       # first section of every third frame
    pairs[1, :, K - 1, 0] = 0.0                     # last section of one utterance
    pairs[2, 42, :, 0] = 0.0                        # every section of the tail block's only frame
    assert int((pairs[..., 0] == 0).sum()) >= 15 + 43 + K - 2
    gy = torch.randn(3, 43, 2 * K, generator=gen)
    got, r64, r32 = _run_ctrl(*_sos_fns("coef"), logits, gy)
    _check_ctrl(SOS_WORST, f"sos2lpc coef zero logits K{K}", got, r64, r32, _sos_tol(K), CAP_COEF)


@pytest.mark.parametrize("rep", ["coef", "conj", "real"])
@pytest.mark.parametrize("K", [11, 32])
def test_sos2lpc_saturated_logits(rep, K):
    gen = torch.Generator().manual_seed(7000 + 10 * K + len(rep))
    logits = torch.randn(3, 43, 2 * K, generator=gen) * 5
    gy = torch.randn(3, 43, 2 * K, generator=gen)
    got, r64, _ = _run_ctrl(*_sos_fns(rep), logits, gy)
    _check_ctrl_global(SOS_WORST, f"sos2lpc saturated {rep} K{K}", got, r64, _sos_tol(K))


@pytest.mark.parametrize("which", ["rc2lpc", "rc2lpc_plain", "coef", "real"])
def test_ctrl_layouts_are_bit_identical(which):
    """A non-contiguous logits view and a non-contiguous incoming gradient give the bits of the contiguous call."""
    from golf_amd import functional as GF

    fn = {"rc2lpc": lambda x: GF.rc2lpc_logits(x, 0.99), "rc2lpc_plain": GF.rc2lpc}.get(which) or _sos_fns(which)[0]
    gen = torch.Generator().manual_seed(8000 + len(which))
    base = (torch.randn(43, 3, 26, generator=gen) * 0.4).cuda()
    gbase = torch.randn(43, 3, 26, generator=gen).cuda()
    x_nc, g_nc = base.transpose(0, 1), gbase.transpose(0, 1)
    assert not x_nc.is_contiguous() and not g_nc.is_contiguous()
    outs = []
    for x, g in ((x_nc, g_nc), (x_nc.contiguous(), g_nc.contiguous())):
        x = x.detach().requires_grad_(True)
        a = fn(x)
        a.backward(g)
        outs.append((a.detach(), x.grad))
    assert outs[0][0].shape == (3, 43, 26)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
