"""The mel-cepstral design kernel (csrc/mlsa_design.hip) and LTVMLSAFilter2 on the device: the basis against numpy float64,
rows and their gradient against tests/mlsa_ref.py over every tile edge, row independence bit for bit, the module against the
reference's own runs (g31), the MLSA decoder streamed against its one-shot forward, one training step of the converted
config, and the refusals.

Bound of the rows and of g_mc: twice the error of the fp32 torch composition on the CPU (the reference's arithmetic width)
against float64 on the same seeded inputs, over the whole grid of cases below -- ``python tests/test_gpu_mlsa.py`` measures it
and prints the two constants; the factor 2 covers another summation order and a device exp / sincos within a couple of ulp.
Bound of the module tests: the bar of the neighbouring LTVCepFilter tests, 1e-4 rel-max and L2 (conftest.rel_err)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import mlsa_ref
from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

NS = (64, 128, 1024, 2048)
MS = (0, 1, 24, 63, 64)
ALPHAS = (0.0, 0.46, -0.3, 0.77)
RS = (1, 2, 17, 63, 64, 65, 130)      # 17: one past the forward's 16-row tile; the backward's tiles are 8 and 4 rows
R_MAX = max(RS)
# measured on the CPU over NS x MS x ALPHAS, 130 rows each (python tests/test_gpu_mlsa.py):
TORCH_FP32_ROWS = 6.02e-06             # max |H - H64| / |H64| per element of the fp32 torch composition
TORCH_FP32_GRAD = 1.08e-04             # max over rows of max|g - g64| / max|g64|
BAR = 1e-4


def _case(n, M, alpha):
    """130 rows: mc[0] in U(-3, 3), mc[m] = N(0, 1) 0.8^m (|Re L| up to about 20: inside the range of fp32 exp), and a
    complex cotangent; rounded to fp32 before anything is computed from them."""
    rng = np.random.default_rng([n, M, int(round(alpha * 100)) + 100])
    mc = rng.normal(0, 1, (R_MAX, M + 1)) * 0.8 ** np.arange(M + 1)
    mc[:, 0] = rng.uniform(-3, 3, R_MAX)
    g_h = rng.normal(0, 1, (R_MAX, n // 2 + 1)) + 1j * rng.normal(0, 1, (R_MAX, n // 2 + 1))
    return mc.astype(np.float32), g_h.astype(np.complex64)


def _row_err(h, h64):
    return float((np.abs(h - h64) / np.abs(h64)).max())


def _grad_err(g, g64):
    return float((np.abs(g - g64).max(axis=-1) / np.abs(g64).max(axis=-1)).max())


def _torch_fp32_errors():
    """The two constants above: the named torch composition in fp32 on the CPU against the float64 definition."""
    from golf_amd import functional as GF

    rows = grad = 0.0
    for n in NS:
        for M in MS:
            for alpha in ALPHAS:
                mc, g_h = _case(n, M, alpha)
                t = torch.from_numpy(mc).requires_grad_()
                h = GF.mel_cepstrum_response_torch(t, n, alpha)
                (g,) = torch.autograd.grad(h, t, torch.from_numpy(g_h))
                rows = max(rows, _row_err(h.detach().numpy(), mlsa_ref.response(mc, n, alpha)))
                grad = max(grad, _grad_err(g.numpy(), mlsa_ref.response_bwd(g_h, mc, n, alpha)))
    return rows, grad


def _basis_views(basis, n, M):
    kp = n // 2 + 64
    b = basis.cpu().numpy().reshape(2, M + 1, kp)
    return b[0], b[1]


@pytest.mark.parametrize("n", NS)
def test_basis_against_numpy_float64(n):
    from golf_amd import functional as GF

    K = n // 2 + 1
    for M in MS:
        for alpha in ALPHAS + (-0.99,):
            c, s = _basis_views(GF.mel_cepstrum_basis(n, M, alpha, "cuda"), n, M)
            c64, s64 = mlsa_ref.tables(n, M, alpha)
            ec, es = np.abs(c[:, :K] - c64).max(), np.abs(s[:, :K] - s64).max()
            assert ec <= 1.2e-7 and es <= 1.2e-7, (n, M, alpha, ec, es)      # 1 fp32 ulp at 1
            assert np.all(s[:, 0] == 0) and np.all(s[:, K - 1] == 0)           # exactly: H is real at DC and Nyquist
            assert np.all(c[:, K:] == 0) and np.all(s[:, K:] == 0)             # the padding columns
    print(f"n {n}: last basis error cos {ec:.2e} sin {es:.2e}")


def _rows(mc, basis, n):
    from golf_amd import functional as GF

    return GF.mel_cepstrum_rows(mc, basis, n)


def _grad(g_h, mc, basis, n):
    from golf_amd import functional as GF

    t = mc.detach().clone().requires_grad_()
    h = GF.mel_cepstrum_response(t, n, 0.0, basis=basis)      # alpha lives in the basis
    (g,) = torch.autograd.grad(h, t, g_h)
    return g


@pytest.mark.parametrize("n", NS)
def test_rows_and_gradient_against_float64(n):
    """Every M, alpha and R of the grid; the rows of a call of R are the first R of the case."""
    from golf_amd import functional as GF

    worst = [0.0, 0.0]
    for M in MS:
        for alpha in ALPHAS:
            mc_np, gh_np = _case(n, M, alpha)
            h64, g64 = mlsa_ref.response(mc_np, n, alpha), mlsa_ref.response_bwd(gh_np, mc_np, n, alpha)
            mc, g_h = torch.from_numpy(mc_np).cuda(), torch.from_numpy(gh_np).cuda()
            basis = GF.mel_cepstrum_basis(n, M, alpha, "cuda")
            for R in RS:
                h = _rows(mc[:R], basis, n)
                assert h.shape == (R, n // 2 + 1) and h.dtype == torch.complex64
                hn = h.cpu().numpy()
                assert np.all(hn.imag[:, [0, -1]] == 0), (n, M, alpha, R)
                g = _grad(g_h[:R], mc[:R], basis, n).cpu().numpy()
                assert g.shape == (R, M + 1)
                er, eg = _row_err(hn, h64[:R]), _grad_err(g, g64[:R])
                worst = [max(worst[0], er), max(worst[1], eg)]
                assert er <= 2 * TORCH_FP32_ROWS, (n, M, alpha, R, er)
                assert eg <= 2 * TORCH_FP32_GRAD, (n, M, alpha, R, eg)
    print(f"n {n}: rows {worst[0]:.3e} (bound {2 * TORCH_FP32_ROWS:.3e}), g_mc {worst[1]:.3e} (bound {2 * TORCH_FP32_GRAD:.3e})")


@pytest.mark.parametrize("n,M,alpha", [(64, 24, 0.46), (1024, 24, 0.46), (2048, 64, 0.77)])
def test_rows_are_independent_of_the_call(n, M, alpha):
    """The rows of a call with R = 130 are, bit for bit, the same rows computed in calls of 1, 64 and 65 rows wherever those
    sit; two runs of the backward are bit-identical, and so is the backward of a part of the rows."""
    from golf_amd import functional as GF

    mc_np, gh_np = _case(n, M, alpha)
    mc, g_h = torch.from_numpy(mc_np).cuda(), torch.from_numpy(gh_np).cuda()
    basis = GF.mel_cepstrum_basis(n, M, alpha, "cuda")
    whole = torch.view_as_real(_rows(mc, basis, n))
    for lo, cnt in ((0, 1), (37, 1), (129, 1), (0, 64), (66, 64), (1, 65), (65, 65)):
        part = torch.view_as_real(_rows(mc[lo:lo + cnt], basis, n))
        assert torch.equal(part, whole[lo:lo + cnt]), (lo, cnt)
    g1, g2 = _grad(g_h, mc, basis, n), _grad(g_h, mc, basis, n)
    assert torch.equal(g1, g2) and torch.isfinite(g1).all()
    assert torch.equal(_grad(g_h[3:68], mc[3:68], basis, n), g1[3:68])
    # module-shaped input (B, F, M + 1) and an empty one
    h3 = GF.mel_cepstrum_response(mc.view(2, 65, M + 1), n, alpha, basis=basis)
    assert h3.shape == (2, 65, n // 2 + 1) and torch.equal(torch.view_as_real(h3).view_as(whole), whole)
    assert GF.mel_cepstrum_response(mc[:0].view(2, 0, M + 1), n, alpha, basis=basis).shape == (2, 0, n // 2 + 1)
    # without a basis of the caller's the function builds one: the same bits
    assert torch.equal(torch.view_as_real(GF.mel_cepstrum_response(mc, n, alpha)), whole)


def _run(m, ex, mc, hop, gy):
    from golf_amd.audiotensor import AudioTensor as AT

    ex, mc = ex.detach().clone().requires_grad_(), mc.detach().clone().requires_grad_()
    y = m(AT(ex), AT(mc, hop)).as_tensor()
    y.backward(gy.to(y))
    return y.detach(), ex.grad, mc.grad


@pytest.mark.parametrize("tag", ["a", "b"])
def test_module_on_the_device_matches_the_references_own_run(golden, tag, monkeypatch):
    from golf_amd import functional as GF
    from golf_amd.filters import LTVMLSAFilter2

    g = golden("g31_mlsa_filter")
    n, hop, M, alpha = (int(g[f"{tag}_n_fft"]), int(g[f"{tag}_hop"]), int(g[f"{tag}_order"]), float(g[f"{tag}_alpha"]))
    flt = LTVMLSAFilter2(n, hop, M, window="hanning", alpha=alpha).cuda()
    calls = []
    rows_op, frames_op = GF._MelCepstrumRows.apply, GF.stft_filter_frames
    monkeypatch.setattr(GF._MelCepstrumRows, "apply", lambda *a: calls.append("rows") or rows_op(*a))
    monkeypatch.setattr(GF, "stft_filter_frames", lambda *a: calls.append("frames") or frames_op(*a))
    ex, mc = torch.from_numpy(g[f"{tag}_ex"]).float().cuda(), torch.from_numpy(g[f"{tag}_mc"]).float().cuda()
    gy = torch.from_numpy(g[f"{tag}_gy"]).float().cuda()
    y, g_ex, g_mc = _run(flt, ex, mc, hop, gy)
    assert calls == ["rows", "frames"] and y.dtype == torch.float32      # both kernels, no torch composition
    assert flt._basis is not None and flt._basis.is_cuda and "_basis" not in flt.state_dict()
    for name, got in (("y", y), ("g_ex", g_ex), ("g_mc", g_mc)):
        emax, el2 = rel_err(got.cpu().numpy(), g[f"{tag}_{name}"])
        print(f"g31{tag} {name}: device module vs the reference's run rel-max {emax:.3e} L2 {el2:.3e}")
        assert emax <= BAR and el2 <= BAR, (tag, name, emax, el2)
    frames = min(1 + ex.shape[1] // hop, mc.shape[1])
    if mc.shape[1] > frames:                                             # control rows no frame uses: zero gradient
        assert torch.all(g_mc[:, frames:] == 0) and g_mc[:, :frames].abs().max() > 0
    # hip_frames = False: the torch composition of the rows is not used on the device either, only the framing is stock
    stock = copy.deepcopy(flt)
    stock.hip_frames = False
    ys, sx, sm = _run(stock, ex, mc, hop, gy)
    assert calls == ["rows", "frames", "rows"]
    for got, own in ((y, ys), (g_ex, sx), (g_mc, sm)):
        emax, el2 = rel_err(got.cpu().numpy(), own.cpu().numpy())
        assert emax <= BAR and el2 <= BAR


def test_module_falls_back_to_torch_where_the_kernel_does_not_reach(monkeypatch):
    """n_fft = 1000 and float64 on the device: the torch composition and torch.stft / torch.istft, against float64 on the CPU."""
    from golf_amd import functional as GF
    from golf_amd.filters import LTVMLSAFilter2

    calls = []
    rows_op = GF._MelCepstrumRows.apply
    monkeypatch.setattr(GF._MelCepstrumRows, "apply", lambda *a: calls.append("rows") or rows_op(*a))
    gen = torch.Generator().manual_seed(1000)
    flt = LTVMLSAFilter2(1000, 250, 12, alpha=0.3).cuda()
    ex = torch.randn(2, 1300, generator=gen).cuda()
    mc = (torch.randn(2, 6, 13, generator=gen) * 0.3 * 0.8 ** torch.arange(13)).cuda()
    gy = torch.randn(2, 1250, generator=gen)
    y, g_ex, g_mc = _run(flt, ex, mc, 250, gy.cuda())
    assert calls == [] and flt._basis is None and y.shape == (2, 1250)
    y64, gx64, gm64 = _run(copy.deepcopy(flt).cpu().double(), ex.cpu().double(), mc.cpu().double(), 250, gy.double())
    for got, ref in ((y, y64), (g_ex, gx64), (g_mc, gm64)):
        emax, el2 = rel_err(got.cpu().numpy(), ref.numpy())
        assert emax <= BAR and el2 <= BAR, (emax, el2)
    f64 = LTVMLSAFilter2(256, 64, 12, alpha=0.3).cuda().double()
    _run(f64, torch.randn(1, 400, dtype=torch.float64).cuda(), torch.zeros(1, 7, 13, dtype=torch.float64).cuda(), 64,
         torch.ones(1, 384, dtype=torch.float64).cuda())
    assert calls == []


# ---- the decoder -----------------------------------------------------------------------------------------------------------
def _model(n=None, hop=None):
    from golf_amd.config import build_model, mlsa_to_stft_filter

    with open(os.path.join(GOLDEN, "g31_mlsa_config.json")) as f:
        cfg = mlsa_to_stft_filter(json.load(f))
    if n is not None:
        cfg["model"]["init_args"]["decoder"]["init_args"]["end_filter"]["init_args"].update(n_fft=n, frame_period=hop)
    return build_model(cfg)


def test_mlsa_decoder_streams_the_bits_of_its_one_shot_forward():
    """The decoder of the converted config at n_fft 64, hop 16; B 2, 12 frames of mel cepstra.  Three cuts -- whole tracks in
    one push, one frame per push, uneven slices with an empty push -- give the same bits as the one-shot forward."""
    from golf_amd.audiotensor import AudioTensor as AT
    from golf_amd.filters import LTVMLSAFilter2
    from golf_amd.stream import SpectralDecoderStream, open_stream
    from golf_amd.synthetic import make_inputs
    from test_gpu_stream_stft import _fixed_noise

    B, hop, F = 2, 16, 12
    T = hop * F
    dec = _model(64, hop).decoder.cuda().eval()
    assert type(dec.end_filter) is LTVMLSAFilter2 and dec.end_filter.n_fft == 64
    base = make_inputs(B=B, T=T, hop=hop, seed=31, with_noise_filter=True, device="cuda")
    gen = torch.Generator().manual_seed(31)
    mc = (torch.randn(B, F, 25, generator=gen) * 0.3 * 0.8 ** torch.arange(25)).cuda()
    with torch.no_grad():
        dec.room_filter.kernel.copy_(base["room_kernel"])
    dec.noise_generator = _fixed_noise(base["noise"])
    x = {"phase": base["phase"], "log_mag": base["log_mag"], "ctrl": mc, "noise": base["noise"]}
    hops = {"phase": 1, "log_mag": hop, "ctrl": hop, "noise": 1}

    def args(sl):
        return dict(phase=AT(sl["phase"]), harm_oscillator_params=(), noise_filter_params=(AT(sl["log_mag"], hop),),
                    end_filter_params=(AT(sl["ctrl"], hop),))

    with torch.no_grad():
        one = dec(noise_generator_params=(), **args(x)).as_tensor()
    assert one.shape[0] == B and one.shape[1] > 0 and one.abs().max() > 0

    def stream(cuts):
        """cuts: per push, the number of frames (of both frame-rate tracks) and of samples it brings"""
        st = open_stream(dec, B)
        assert type(st) is SpectralDecoderStream
        pos = dict.fromkeys(x, 0)
        outs = []
        for nf, ns in cuts:
            sl = {}
            for k in x:
                m = ns if hops[k] == 1 else nf
                sl[k] = x[k][:, pos[k]: pos[k] + m]
                pos[k] = min(pos[k] + m, x[k].shape[1])
            outs.append(st.push(**args(sl), noise=AT(sl["noise"])))
        assert all(pos[k] == x[k].shape[1] for k in x)
        outs.append(st.finish())
        return torch.cat(outs, 1)

    cuts = ([(F, T)],
            [(1, hop)] * F,
            [(0, 7), (3, 0), (0, 0), (1, 41), (5, 100), (3, T - 148)])
    for c in cuts:
        y = stream(c)
        assert y.shape == one.shape, (c, y.shape, one.shape)
        assert torch.equal(y, one), (c, (y - one).abs().max())


def test_one_training_step_of_the_converted_config():
    """B 2, T 4800: the loss is finite, the encoder head gets a gradient, and what the end filter computed inside the step --
    output, gradient of the excitation, gradient of the mel cepstra -- is the float64 CPU module's on the same inputs."""
    from golf_amd.filters import LTVMLSAFilter2

    torch.manual_seed(31)
    B, T = 2, 4800
    model = _model().cuda().train()
    flt = model.decoder.end_filter
    assert type(flt) is LTVMLSAFilter2 and (flt.n_fft, flt.hop_length) == (1024, 240)
    seen = {}

    def hook(module, inputs, output):
        seen["ex"], seen["mc"], seen["y"] = inputs[0].as_tensor(), inputs[1].as_tensor(), output.as_tensor()
        for v in seen.values():
            v.retain_grad()

    handle = flt.register_forward_hook(hook)
    t = torch.arange(T, device="cuda") / 24000
    f0 = (120 + 40 * torch.rand(B, 1, device="cuda")) * (1 + 0.03 * torch.sin(2 * np.pi * 5.5 * t))[None]
    x = 0.1 * torch.sin(2 * np.pi * torch.cumsum(f0 / 24000, 1)) + 0.01 * torch.randn(B, T, device="cuda")
    loss = model.training_step((x, f0), unvoiced_f0=torch.full((B, 1), 200.0, device="cuda"))
    loss.backward()
    handle.remove()
    assert torch.isfinite(loss)
    head = model.encoder.backbone.out_linear.weight.grad
    assert head is not None and torch.isfinite(head).all() and head.abs().max() > 0
    assert seen["mc"].shape[2] == 25 and seen["mc"].grad.abs().max() > 0
    y64, gx64, gm64 = _run(copy.deepcopy(flt).cpu().double(), seen["ex"].cpu().double(), seen["mc"].cpu().double(), 240,
                           seen["y"].grad.cpu().double())
    for name, got, ref in (("y", seen["y"].detach(), y64), ("g_ex", seen["ex"].grad, gx64), ("g_mc", seen["mc"].grad, gm64)):
        emax, el2 = rel_err(got.cpu().numpy(), ref.numpy())
        print(f"training step, end filter {name}: device vs float64 CPU module rel-max {emax:.3e} L2 {el2:.3e}")
        assert emax <= BAR and el2 <= BAR, (name, emax, el2)


def test_refusals_raise_before_any_launch():
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError, load

    with pytest.raises(GolfError, match="order"):
        GF.mel_cepstrum_basis(1024, 65, 0.46, "cuda")
    with pytest.raises(GolfError, match="power of two"):
        GF.mel_cepstrum_basis(1000, 24, 0.46, "cuda")
    for alpha in (1.0, -1.0, 1.3):
        with pytest.raises(GolfError, match="alpha"):
            GF.mel_cepstrum_basis(1024, 24, alpha, "cuda")
    basis = GF.mel_cepstrum_basis(1024, 24, 0.46, "cuda")
    mc = torch.zeros(4, 25).cuda()
    with pytest.raises(GolfError, match="power of two"):
        GF.mel_cepstrum_rows(mc, basis, 1000)                       # the C entry; the module runs torch at n_fft = 1000
    with pytest.raises(GolfError, match="order"):
        GF.mel_cepstrum_rows(torch.zeros(4, 66).cuda(), basis, 1024)
    with pytest.raises(GolfError, match="bytes"):
        GF.mel_cepstrum_rows(mc, basis[:-1], 1024)                  # a short basis
    with pytest.raises(GolfError, match="no CPU path"):
        GF.mel_cepstrum_rows(mc.cpu(), basis, 1024)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.mel_cepstrum_rows(mc, basis.cpu(), 1024)
    with pytest.raises(GolfError, match="fp32"):
        GF.mel_cepstrum_rows(mc.double(), basis, 1024)
    lib = load()
    h = torch.empty(4, 513, 2).cuda()
    assert lib.golf_mlsa_response_rows_f32(mc.data_ptr(), basis.data_ptr(), basis.numel() * 4, h.data_ptr(), 0, 1024, 24,
                                           None) == 0               # R = 0 does nothing
    torch.cuda.synchronize()


if __name__ == "__main__":
    print("TORCH_FP32_ROWS = %.2e, TORCH_FP32_GRAD = %.2e" % _torch_fp32_errors())
