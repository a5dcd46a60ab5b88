"""GPU parity of the minimum-phase FIR filters (golf_min_phase_fir_* + golf_ltv_fir_frames_causal_*; reference
LTVMinimumPhaseFIRFilter / ...Precise, models/filters.py:198-283), LTIRadiationFilter (:400-423) and
SampleBasedLTVMinimumPhaseFilter (:763-790): golden vectors produced by the reference itself (g29, g30), the float64
restatement (tests/minphase_ref.py) at larger sizes, gradients, and size-independent properties.

Bars: those of the zero-phase twin (tests/test_gpu_noise_fir.py).  The reference's own formula in float32 (FFTs, autograd
on the CPU) sits 8e-8 .. 2.5e-7 (y), 7e-8 .. 2.2e-7 (g_ex) and 9e-8 .. 3.5e-7 (g_log_mag) rel-max from float64 on the
six envelopes of test_fwd_bwd_vs_float64: far under half a bar, so the gradient bars stay at 2e-5."""

import numpy as np
import pytest
import torch

import minphase_ref as R
from conftest import rel_err
from test_gpu_noise_fir import case

pytestmark = pytest.mark.gpu


def dev(x, grad=False):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32).cuda().requires_grad_(grad)


def check(y, ref, what, tol):
    y = np.asarray(y)
    emax, el2 = rel_err(y, ref)
    print(f"{what}: rel-max {emax:.3e} rel-l2 {el2:.3e}")
    assert np.isfinite(y).all()
    assert emax <= tol and el2 <= tol, (what, emax, el2)


def run_module(ex, log_mag, hop, window="hanning", gy=None, precise=False):
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import LTVMinimumPhaseFIRFilter, LTVMinimumPhaseFIRFilterPrecise

    n_mag = log_mag.shape[-1]
    m = (LTVMinimumPhaseFIRFilterPrecise(window=window, n_mag=n_mag) if precise
         else LTVMinimumPhaseFIRFilter(window=window, conv_method="direct", n_mag=n_mag)).cuda()
    x, lm = dev(ex, gy is not None), dev(log_mag, gy is not None)
    y = m(AudioTensor(x), AudioTensor(lm, hop))
    assert y.hop_length == 1
    yt = y.as_tensor()
    if gy is None:
        torch.cuda.synchronize()
        return yt.detach().cpu().numpy()
    (yt * dev(gy)).sum().backward()
    torch.cuda.synchronize()
    return yt.detach().cpu().numpy(), x.grad.cpu().numpy(), lm.grad.cpu().numpy()


# ---------------------------------------------------------------------------------------------- golden g29
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_golden_g29(golden, tag):
    from golf_amd import functional as GF

    g = golden("g29_min_phase_fir")
    ex, lm, hop, window = g[f"{tag}_ex"], g[f"{tag}_log_mag"], int(g[f"{tag}_hop"]), str(g[f"{tag}_window"])
    N = 2 * (lm.shape[-1] - 1)
    k = GF.min_phase_fir_kernels(dev(lm), dev(R.min_phase_window(window, N).numpy())).cpu().numpy()
    check(k, g[f"{tag}_kernel"], f"g29{tag} kernel", 2e-6)
    y, gx, glm = run_module(ex, lm, hop, window, gy=g[f"{tag}_gy"])
    check(y, g[f"{tag}_y"], f"g29{tag} y", 1e-5)
    check(gx, g[f"{tag}_g_ex"], f"g29{tag} g_ex", 1e-5)
    check(glm, g[f"{tag}_g_log_mag"], f"g29{tag} g_log_mag", 1e-5)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_precise_golden_g29(golden, tag):
    g = golden("g29_min_phase_fir")
    ex, lm, hop, window = g[f"{tag}_ex"], g[f"{tag}_log_mag"], int(g[f"{tag}_hop"]), str(g[f"{tag}_window"])
    y, gx, glm = run_module(ex, lm, hop, window, gy=g[f"{tag}_p_gy"], precise=True)
    check(y, g[f"{tag}_p_y"], f"g29{tag} precise y", 1e-5)
    check(gx, g[f"{tag}_p_g_ex"], f"g29{tag} precise g_ex", 1e-5)
    check(glm, g[f"{tag}_p_g_log_mag"], f"g29{tag} precise g_log_mag", 1e-5)


# ---------------------------------------------------------------------------------------------- float64 restatement
@pytest.mark.parametrize("B,T,F,n_mag,hop", [(5, 480, 2, 9, 240), (2, 700, 30, 17, 24), (2, 1500, 20, 33, 64),
                                             (3, 2000, 9, 65, 240), (1, 3000, 5, 129, 600), (2, 999, 3, 256, 240)])
def test_fwd_bwd_vs_float64(B, T, F, n_mag, hop):
    """Two of the shapes, (2, 1500, 20, 33, 64) and (2, 999, 3, 256, 240), hold more frames of excitation than kernels
    (T // hop > F): the reference asserts there and the filter raises.  The test asserts that refusal and then checks the
    numbers on the F * hop samples the F kernels do serve."""
    from golf_amd import _lib

    ex, lm = case(B, T, F, n_mag, seed=T + n_mag)
    if T // hop > F:
        with pytest.raises(_lib.GolfError):
            run_module(ex, lm, hop)
        ex = ex[:, : F * hop]
    win = R.min_phase_window("hanning", 2 * (n_mag - 1))
    gy = np.random.default_rng(7).normal(0, 1, (B, (ex.shape[1] // hop) * hop)).astype(np.float32)
    ref, rgx, rglm = R.filter_with_grads(ex, lm, win, hop, gy)
    y, gx, glm = run_module(ex, lm, hop, gy=gy)
    assert y.shape == ref.shape
    check(y, ref, f"min-phase fwd B{B} T{T} F{F} n_mag{n_mag} hop{hop}", 1e-5)
    check(gx, rgx, "g_ex", 2e-5)          # float32 reference formula: <= 2.2e-7 from float64 on these inputs
    check(glm, rglm, "g_log_mag", 2e-5)   # float32 reference formula: <= 3.5e-7


@pytest.mark.parametrize("B,T,F,n_mag,hop", [(2, 2500, 11, 65, 240), (1, 700, 30, 17, 24)])
def test_precise_vs_float64(B, T, F, n_mag, hop):
    ex, lm = case(B, T, F, n_mag, seed=T + n_mag + 1)
    win = R.min_phase_window("hanning", 2 * (n_mag - 1))
    Tout = min(T, (F - 1) * hop + 1)
    gy = np.random.default_rng(9).normal(0, 1, (B, Tout)).astype(np.float32)
    ref, rgx, rglm = R.filter_with_grads(ex, lm, win, hop, gy, samplewise=True)
    y, gx, glm = run_module(ex, lm, hop, gy=gy, precise=True)
    assert y.shape == ref.shape == (B, Tout)
    check(y, ref, f"precise fwd B{B} T{T} F{F} n_mag{n_mag} hop{hop}", 1e-5)
    check(gx, rgx, "precise g_ex", 2e-5)
    check(glm, rglm, "precise g_log_mag", 2e-5)


def test_full_size_module():
    """The noise branch's shape of the BASELINE config (B=32, 2 s @ 24 kHz, F=200 frames, n_mag=256, hop 240) through the
    module: the float64 restatement on 4 rows of the batch, linearity in the excitation over all of it."""
    B, T, F, n_mag, hop = 32, 48000, 200, 256, 240
    ex, lm = case(B, T, F, n_mag, seed=2434)
    win = R.min_phase_window("hanning", 510)
    gy = np.random.default_rng(11).normal(0, 1, (B, T)).astype(np.float32)
    y, gx, glm = run_module(ex, lm, hop, gy=gy)
    assert y.shape == (B, T)
    nb = 4
    ref, rgx, rglm = R.filter_with_grads(ex[:nb], lm[:nb], win, hop, gy[:nb])
    check(y[:nb], ref, "full-size fwd", 1e-5)
    check(gx[:nb], rgx, "full-size g_ex", 2e-5)
    check(glm[:nb], rglm, "full-size g_log_mag", 2e-5)
    y2 = run_module(2.0 * ex, lm, hop)
    np.testing.assert_allclose(y2, 2.0 * y, rtol=0, atol=1e-5 * np.abs(y).max())  # linear in the excitation


# ---------------------------------------------------------------------------------------------- properties
def test_flat_spectrum_is_the_identity():
    """log_mag = 0 -> theta = 0 -> the kernel is a delta at tap 0: no delay, y == ex."""
    B, T, F, n_mag, hop = 2, 1000, 5, 33, 240
    ex = np.random.default_rng(0).normal(0, 1, (B, T)).astype(np.float32)
    y = run_module(ex, np.zeros((B, F, n_mag), np.float32), hop)
    assert y.shape == (B, 960)
    np.testing.assert_allclose(y, ex[:, :960], rtol=0, atol=2e-6)


@pytest.mark.parametrize("n_mag", [9, 65, 256])
def test_kernel_sums_and_magnitude(n_mag):
    """Window of ones: sum_m h[m] = H(0) = e^{L[0]}, sum_m (-1)^m h[m] = H(N/2) = e^{L[N/2]} (theta vanishes at both),
    and |fft(h)| = exp(log_mag)."""
    from golf_amd import functional as GF

    _, lm = case(3, 8, 7, n_mag, seed=n_mag)
    N = 2 * (n_mag - 1)
    h = GF.min_phase_fir_kernels(dev(lm), torch.ones(N, device="cuda")).cpu().numpy().astype(np.float64)
    assert h.shape == (3, 7, N)
    mag = np.exp(lm.astype(np.float64))
    alt = (-1.0) ** np.arange(N)
    np.testing.assert_allclose(h.sum(-1), mag[..., 0], rtol=0, atol=1e-5 * mag.max())
    np.testing.assert_allclose((h * alt).sum(-1), mag[..., -1], rtol=0, atol=1e-5 * mag.max())
    np.testing.assert_allclose(np.abs(np.fft.rfft(h, axis=-1)), mag, rtol=0, atol=1e-5 * mag.max())


def test_causality():
    """Changing ex[:, t0:] leaves y[:, :t0] bitwise equal (frame-wise and sample-wise)."""
    B, T, F, n_mag, hop = 2, 1400, 12, 33, 120
    ex, lm = case(B, T, F, n_mag, seed=5)
    ex2 = ex.copy()
    t0 = 777
    ex2[:, t0:] = np.random.default_rng(1).normal(0, 1, (B, T - t0))
    for precise in (False, True):
        y, y2 = run_module(ex, lm, hop, precise=precise), run_module(ex2, lm, hop, precise=precise)
        assert np.array_equal(y[:, :t0], y2[:, :t0])
        assert not np.array_equal(y[:, t0:], y2[:, t0:])


def test_unused_frames_get_zero_gradient():
    B, T, F, n_mag, hop = 2, 1000, 9, 33, 240
    ex, lm = case(B, T, F, n_mag, seed=6)
    gy = np.ones((B, 960), np.float32)
    _, _, glm = run_module(ex, lm, hop, gy=gy)
    assert np.all(glm[:, 4:] == 0), "T // hop = 4 frames are filtered: kernels 4.. are never used"
    assert np.all(np.abs(glm[:, :4]).max(-1) > 0)


@pytest.mark.parametrize("n_mag", [9, 100, 256])
def test_padding_taps_are_zero(n_mag):
    """Taps [N, row_stride) are zeros in the kernel rows and in their gradient (buffers poisoned beforehand)."""
    from golf_amd import functional as GF

    B, F, hop = 2, 5, 48
    N = 2 * (n_mag - 1)
    ex, lm = case(B, F * hop, F, n_mag, seed=n_mag)
    lib = GF._lib.load()
    KS = lib.golf_zero_phase_fir_row_stride(n_mag)
    lmd, win = dev(lm), dev(R.min_phase_window("hanning", N).numpy())
    kern = torch.full((B * F, KS), float("nan"), device="cuda")
    GF._lib.check(lib.golf_min_phase_fir_kernels_f32(lmd.data_ptr(), win.data_ptr(),
                                                     GF.min_phase_fir_basis(n_mag, "cuda").data_ptr(), kern.data_ptr(),
                                                     B * F, n_mag, GF._lib.stream_ptr()), "kernels")
    assert torch.isfinite(kern).all() and (kern[:, N:] == 0).all()
    x, gy = dev(ex), dev(np.ones((B, F * hop), np.float32))
    g_kern = torch.full((B * F, KS), float("nan"), device="cuda")
    GF._lib.check(lib.golf_ltv_fir_frames_causal_bwd_f32(gy.data_ptr(), gy.stride(0), x.data_ptr(), x.stride(0),
                                                         kern.data_ptr(), KS, None, 0, g_kern.data_ptr(), B, F * hop, F, N,
                                                         hop, 0, GF._lib.stream_ptr()), "bwd")
    assert torch.isfinite(g_kern).all() and (g_kern[:, N:] == 0).all()
    assert KS == N or g_kern[:, :N].abs().max() > 0


def test_generic_causal_frames_match_torch_conv():
    """ltv_fir_frames_causal with arbitrary kernels against a float64 grouped convolution, values and gradients."""
    from golf_amd import functional as GF

    B, T, F, N, hop = 3, 1111, 14, 30, 80
    rng = np.random.default_rng(3)
    ex, k = rng.normal(0, 1, (B, T)), rng.normal(0, 1, (B, F, N)) / N
    nfr = T // hop
    gy = rng.normal(0, 1, (B, nfr * hop))
    x64, k64 = torch.tensor(ex, requires_grad=True), torch.tensor(k, requires_grad=True)
    ref = R.causal_frames(x64, k64, hop)
    (ref * torch.tensor(gy)).sum().backward()
    x, kk = dev(ex, True), dev(k, True)
    y = GF.ltv_fir_frames_causal(x, kk, hop)
    (y * dev(gy)).sum().backward()
    check(y.detach().cpu().numpy(), ref.detach().numpy(), "causal frames", 1e-5)
    check(x.grad.cpu().numpy(), x64.grad.numpy(), "causal frames g_ex", 1e-5)
    check(kk.grad.cpu().numpy(), k64.grad.numpy(), "causal frames g_kernels", 1e-5)


# ---------------------------------------------------------------------------------------------- errors
def test_errors():
    from golf_amd import _lib
    from golf_amd import functional as GF

    lm = torch.zeros(2, 4, 129, device="cuda")
    win = torch.ones(256, device="cuda")
    with pytest.raises(_lib.GolfError):  # T // hop > F
        GF.min_phase_fir_filter(torch.zeros(2, 1200, device="cuda"), lm, win, 240)
    with pytest.raises(_lib.GolfError):  # T < hop
        GF.min_phase_fir_filter(torch.zeros(2, 100, device="cuda"), lm, win, 240)
    with pytest.raises(_lib.GolfError):  # window / n_mag mismatch
        GF.min_phase_fir_filter(torch.zeros(2, 900, device="cuda"), lm, torch.ones(100, device="cuda"), 240)
    with pytest.raises(_lib.GolfError):
        GF.min_phase_fir_kernels(lm, torch.ones(100, device="cuda"))
    with pytest.raises(_lib.GolfError):  # CPU tensors: there is no CPU path
        GF.min_phase_fir_filter(torch.zeros(2, 900), lm.cpu(), win.cpu(), 240)
    y = GF.min_phase_fir_filter(torch.zeros(2, 486, device="cuda", requires_grad=True), lm, win, 243)
    with pytest.raises(_lib.GolfError, match="must be a multiple of 4"):  # the twin's backward restriction
        y.sum().backward()


# ---------------------------------------------------------------------------------------------- other classes
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_radiation_filter_g30(golden, tag):
    from golf_amd.filters import LTIRadiationFilter

    g = golden("g30_radiation_filter")
    m = LTIRadiationFilter(int(g[f"{tag}_num_zeros"]), window=str(g[f"{tag}_window"])).cuda()
    assert "_kernel" not in m.state_dict() and m._kernel.shape == g[f"{tag}_module_kernel"].shape
    check(m._kernel.cpu().numpy(), g[f"{tag}_module_kernel"], f"g30{tag} kernel", 1e-6)
    x = dev(g[f"{tag}_ex"], True)
    y = m(x)
    assert y.shape == x.shape
    (y * dev(g[f"{tag}_gy"])).sum().backward()
    check(y.detach().cpu().numpy(), g[f"{tag}_y"], f"g30{tag} y", 1e-5)
    check(x.grad.cpu().numpy(), g[f"{tag}_g_ex"], f"g30{tag} g_ex", 1e-5)


def test_sample_based_filter_is_the_precise_filter():
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import LTVMinimumPhaseFilter, LTVMinimumPhaseFilterPrecise, SampleBasedLTVMinimumPhaseFilter
    from golf_amd.synthetic import make_inputs

    with pytest.warns(UserWarning, match="SampleBasedLTVMinimumPhaseFilter is deprecated"):
        old = SampleBasedLTVMinimumPhaseFilter(lpc_order=22).cuda()
    assert isinstance(old, LTVMinimumPhaseFilter)
    new = LTVMinimumPhaseFilterPrecise(lpc_order=22).cuda()
    assert old.ctrl.split_size == new.ctrl.split_size == (1, 22)
    inp = make_inputs(B=2, T=4800, device="cuda")
    outs = []
    for f in (old, new):
        ex, a = inp["noise"].clone().requires_grad_(True), inp["a"].clone().requires_grad_(True)
        y = f(AudioTensor(ex), AudioTensor(inp["gain"], 240), AudioTensor(a, 240)).as_tensor()
        y.square().mean().backward()
        outs.append((y.detach(), ex.grad, a.grad))
    for u, v in zip(*outs):
        assert torch.equal(u, v)


DECODER = """
decoder:
  class_path: models.sf.SourceFilterSynth
  init_args:
    harm_oscillator:
      class_path: models.synth.DownsampledIndexedGlottalFlowTable
      init_args: {hop_rate: 10, in_channels: 64, oversampling: 4, equal_energy: true, table_size: 100,
                  table_type: derivative, normalize_method: constant_power, align_peak: true, trainable: false,
                  min_R_d: 0.3, max_R_d: 2.7, lf_v2: true, points: 2048}
    noise_generator: {class_path: models.noise.StandardNormalNoise}
    noise_filter:
      class_path: models.filters.LTVMinimumPhaseFIRFilter
      init_args: {window: hanning, conv_method: direct, n_mag: 33}
    end_filter:
      class_path: models.filters.LTVMinimumPhaseFilterPrecise
      init_args: {lpc_order: 22, lpc_parameterisation: rc2lpc}
    subtract_harmonics: false
"""


def test_yaml_decoder_with_min_phase_noise_filter():
    """A SourceFilterSynth built from YAML with the minimum-phase FIR as its noise filter runs forward and backward and is
    the composition of its parts."""
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.config import build_model
    from golf_amd.filters import LTVMinimumPhaseFIRFilter
    from golf_amd.synthetic import make_inputs

    dec = build_model(DECODER).cuda()
    assert type(dec.noise_filter) is LTVMinimumPhaseFIRFilter
    assert dec.split_sizes_and_trsfms[0] == ((64,), (), (33,), (1, 22), ())
    inp = make_inputs(B=2, T=4800, device="cuda", with_noise_filter=True, n_mag=33)
    lm = inp["log_mag"].clone().requires_grad_(True)
    a = inp["a"].clone().requires_grad_(True)
    phase, w = AudioTensor(inp["phase"]), AudioTensor(inp["wsel"], inp["w_hop"])
    gain = AudioTensor(inp["gain"], 240)
    torch.manual_seed(3)
    y = dec(phase=phase, harm_oscillator_params=(w,), noise_generator_params=(),
            noise_filter_params=(AudioTensor(lm, 240),), end_filter_params=(gain, AudioTensor(a, 240))).as_tensor()
    y.square().mean().backward()
    assert torch.isfinite(y).all() and torch.isfinite(lm.grad).all() and lm.grad.abs().max() > 0 and a.grad.abs().max() > 0
    with torch.no_grad():
        torch.manual_seed(3)
        harm = dec.harm_oscillator(phase, w)
        nz = dec.noise_filter(dec.noise_generator(harm), AudioTensor(inp["log_mag"], 240))
        ref = dec.end_filter(harm + nz, gain, AudioTensor(inp["a"], 240)).as_tensor()
    assert ref.shape == y.shape
    check(y.detach().cpu().numpy(), ref.cpu().numpy(), "decoder vs composition", 1e-5)
