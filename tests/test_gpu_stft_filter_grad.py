"""The differentiable STFT-domain frame filter on the device: golf_stft_filter_frames_bwd_f32 behind GF.stft_filter_frames
against the float64 closed form (tests/stft_filter_ref.py) and float64 CPU autograd through torch.stft / torch.istft; bit
reproducibility; the forward's bits; LTVCepFilter / DiffWorldSPFilter routed through it; the shipped NHV and WORLD decoders
trained through it; hipGraph capture.

Bound: the project's parity bar, 1e-4 rel-max and L2 (conftest.rel_err), the bar of the forward's tests.  Every comparison
prints the kernel's distances next to those of torch's own fp32 autograd on the device."""
import copy

import numpy as np
import pytest
import torch

import stft_filter_ref as R
from conftest import rel_err
from test_gpu_stream_stft import _call_args, _cep, _decoder, _fixed_noise, _inputs, _response

pytestmark = pytest.mark.gpu

BAR = 1e-4
# log2 n even and odd; the shared 64-lane block; 512 lanes; one frame per block of n/4 lanes from 256 on: a single wave (256)
# and two waves with a radix-2 last stage (512)
GEOMETRIES = [(64, 24), (128, 32), (256, 60), (512, 120), (1024, 240), (2048, 600)]


def _np(t):
    """float64 numpy, a complex tensor as (..., 2)."""
    t = t.detach().cpu()
    return (torch.view_as_real(t.to(torch.complex128)) if t.is_complex() else t.double()).numpy()


def _rows(kind, B, F, n, gen):
    if kind == "complex":
        return torch.complex(1 + 0.3 * torch.randn(B, F, n // 2 + 1, generator=gen), 0.3 * torch.randn(B, F, n // 2 + 1, generator=gen))
    return torch.exp(0.3 * torch.randn(B, F, n // 2 + 1, generator=gen))


def _torch_filter(x, H, w, hop):
    """The reference's arithmetic: torch.stft -> product with the rows -> torch.istft (one-sided: the Hermitian extension)."""
    n = w.numel()
    X = torch.stft(x, n, hop, n, w, center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    frames = min(X.shape[-1], H.shape[1])
    Y = X[..., :frames] * H[:, :frames].transpose(1, 2)
    return torch.istft(Y, n, hop, n, w, center=True, normalized=False, onesided=True, return_complex=False)


def _grads(fn, x, H, w, hop, gy):
    x, H = x.detach().clone().requires_grad_(), H.detach().clone().requires_grad_()
    y = fn(x, H, w, hop)
    y.backward(gy.to(y.dtype))
    return y.detach(), x.grad, H.grad


def _compare(what, got, own, ref):
    """Assert `got` within the bar of the float64 `ref`; print it next to torch's own fp32 result `own`."""
    k, o = rel_err(_np(got), ref), rel_err(_np(own), ref)
    print(f"{what}: kernel vs float64 rel-max {k[0]:.3e} L2 {k[1]:.3e}; torch fp32 autograd on the device {o[0]:.3e} {o[1]:.3e}")
    assert k[0] <= BAR and k[1] <= BAR, (what, k)


@pytest.mark.parametrize("n,hop", GEOMETRIES)
def test_op_gradients_against_float64(n, hop):
    """B = 3; T = 5 hop + 7, 6 hop and n/2 + 8 (a frame reflecting at both ends); F on both sides of 1 + T // hop; complex
    and real rows; a random gy."""
    from golf_amd import functional as GF

    gen = torch.Generator().manual_seed(7 * n + hop)
    w = torch.hann_window(n)
    for kind in ("complex", "real"):
        for T in (5 * hop + 7, 6 * hop, n // 2 + 8):
            for F in (max(2, T // hop), T // hop + 3):
                frames = min(1 + T // hop, F)
                x, H = torch.randn(3, T, generator=gen), _rows(kind, 3, F, n, gen)
                gy = torch.randn(3, hop * (frames - 1), generator=gen)
                y64, gx64, gH64 = _grads(_torch_filter, x.double(), H.to(torch.complex128 if kind == "complex" else torch.float64),
                                         w.double(), hop, gy.double())
                gxr, gHr = R.backward(gy.numpy(), x.numpy(), H.numpy(), w.double().numpy(), hop)
                # the two float64 references agree far below the bar
                assert rel_err(gxr, _np(gx64))[0] <= 1e-12 and rel_err(_np(torch.from_numpy(gHr)), _np(gH64))[0] <= 1e-12
                y, gx, gH = _grads(GF.stft_filter_frames, x.cuda(), H.cuda(), w.cuda(), hop, gy.cuda())
                _, ox, oH = _grads(_torch_filter, x.cuda(), H.cuda(), w.cuda(), hop, gy.cuda())
                tag = f"{kind} n {n} hop {hop} T {T} F {F}"
                assert gx.shape == x.shape and gH.shape == H.shape and gx.dtype == torch.float32 and gH.dtype == H.dtype
                assert torch.isfinite(gx).all() and torch.isfinite(torch.view_as_real(gH) if gH.is_complex() else gH).all()
                assert not _np(gH[:, frames:]).any(), tag           # the rows no frame uses: exactly zero
                _compare(tag + " y", y, y, _np(y64))
                for name, got, own, refs in (("g_x", gx, ox, (gxr, _np(gx64))), ("g_H", gH, oH, (_np(torch.from_numpy(gHr)), _np(gH64)))):
                    for ref in refs:
                        _compare(f"{tag} {name}", got, own, ref)


@pytest.mark.parametrize("n,hop", [(64, 24), (1024, 240)])
def test_gradients_are_bit_reproducible_and_independent_of_each_other(n, hop):
    from golf_amd import functional as GF

    gen = torch.Generator().manual_seed(n)
    w = torch.hann_window(n).cuda()
    T, F = 5 * hop + 7, 9
    for kind in ("complex", "real"):
        x, H = torch.randn(3, T, generator=gen).cuda(), _rows(kind, 3, F, n, gen).cuda()
        gy = torch.randn(3, hop * 5, generator=gen).cuda()
        _, gx, gH = _grads(GF.stft_filter_frames, x, H, w, hop, gy)
        _, gx2, gH2 = _grads(GF.stft_filter_frames, x, H, w, hop, gy)
        eq = lambda a, b: torch.equal(torch.view_as_real(a), torch.view_as_real(b)) if a.is_complex() else torch.equal(a, b)
        assert eq(gx, gx2) and eq(gH, gH2)
        xr = x.clone().requires_grad_()
        GF.stft_filter_frames(xr, H, w, hop).backward(gy)
        assert eq(xr.grad, gx)
        Hr = H.clone().requires_grad_()
        GF.stft_filter_frames(x, Hr, w, hop).backward(gy)
        assert eq(Hr.grad, gH)


def test_a_single_frame_reaches_no_sample_and_gives_zero_gradients():
    from golf_amd import functional as GF

    gen = torch.Generator().manual_seed(2)
    w = torch.hann_window(64).cuda()
    for kind in ("complex", "real"):
        x, H = torch.randn(3, 200, generator=gen).cuda().requires_grad_(), _rows(kind, 3, 1, 64, gen).cuda().requires_grad_()
        y = GF.stft_filter_frames(x, H, w, 24)
        assert y.shape == (3, 0)
        y.sum().backward()
        assert x.grad.shape == x.shape and H.grad.shape == H.shape and not _np(x.grad).any() and not _np(H.grad).any()


@pytest.mark.parametrize("n,hop", [(128, 32), (1024, 240)])
def test_forward_bits_are_the_streaming_entrys(n, hop):
    from golf_amd import functional as GF

    gen = torch.Generator().manual_seed(n + 1)
    w = torch.hann_window(n).cuda()
    T, F = 6 * hop, 8
    for kind in ("complex", "real"):
        x, H = torch.randn(3, T, generator=gen).cuda(), _rows(kind, 3, F, n, gen).cuda()
        frames = min(1 + T // hop, F)
        want = GF.stft_filter_stream(x, H, w, hop, None, x0=0, h0=0, f0=0, nf=frames, n0=0, ny=hop * (frames - 1), x_end=T,
                                     frames_end=frames)[0]
        with torch.no_grad():
            assert torch.equal(GF.stft_filter_frames(x, H, w, hop), want)
        y = GF.stft_filter_frames(x, H, w, hop)              # grad mode on, nothing requires grad
        assert torch.equal(y, want) and not y.requires_grad
        y = GF.stft_filter_frames(x.clone().requires_grad_(), H, w, hop)
        assert torch.equal(y, want) and y.requires_grad


def _world(n, hop):
    from golf_amd.filters import DiffWorldSPFilter

    # f_max 4400, not 4000: with 4000 the rectified pseudo-inverse filterbank has an all-zero Nyquist column and the sqrt makes
    # the reference's own gradient w.r.t. mel_sp NaN in float64
    return DiffWorldSPFilter(n_mels=12, n_fft=n, hop_length=hop, f_min=0.0, f_max=4400.0, center=True, window="hanning",
                             sample_rate=8000, norm=None, mel_scale="htk")


@pytest.mark.parametrize("kind", ["min", "zero", "world"])
def test_modules_run_and_train_on_the_kernel(kind, monkeypatch):
    from golf_amd import functional as GF
    from golf_amd.audiotensor import AudioTensor as AT

    n, hop, B = 128, 32, 3
    T = 6 * hop + 7
    F = T // hop + 3
    gen = torch.Generator().manual_seed(11)
    flt = (_world(n, hop) if kind == "world" else _cep(n, hop, kind)).cuda()
    x = torch.randn(B, T, generator=gen).cuda()
    if kind == "world":
        ctrl = torch.exp(0.3 * torch.randn(B, F, 12, generator=gen) - 2).cuda()
    else:
        ctrl = (torch.randn(B, F, 25, generator=gen) * 0.2 / (1 + torch.arange(25))).cuda()
    gy = torch.randn(B, hop * (T // hop), generator=gen)

    def run(m, xx, cc, g):
        xx, cc = xx.detach().clone().requires_grad_(), cc.detach().clone().requires_grad_()
        y = m(AT(xx), AT(cc, hop)).as_tensor()
        y.backward(g.to(y))
        return y.detach(), xx.grad, cc.grad

    calls = []
    frames_op = GF.stft_filter_frames
    monkeypatch.setattr(GF, "stft_filter_frames", lambda *a: calls.append(1) or frames_op(*a))
    y, gx, gc = run(flt, x, ctrl, gy.cuda())
    assert calls == [1] and y.dtype == torch.float32
    # the routed module is the op on the stream's own rows, bit for bit
    assert torch.equal(y, frames_op(x, _response(flt, ctrl), flt._window, hop))
    stock = copy.deepcopy(flt)
    stock.hip_frames = False
    ys, sx, sc = run(stock, x, ctrl, gy.cuda())
    assert calls == [1] and ys.shape == y.shape       # hip_frames = False: torch.stft / torch.istft on the device
    y64, gx64, gc64 = run(copy.deepcopy(flt).cpu().double(), x.cpu().double(), ctrl.cpu().double(), gy.double())
    assert torch.isfinite(gc64).all()
    for name, got, own, ref in (("y", y, ys, y64), ("g_ex", gx, sx, gx64), ("g_ctrl", gc, sc, gc64)):
        _compare(f"{kind} module {name}", got, own, _np(ref))
    # float64 on the device and an unsupported geometry keep the stock path
    run(copy.deepcopy(flt).double(), x.double(), ctrl.double(), gy.cuda().double())
    assert calls == [1]


@pytest.mark.parametrize("name", ["nhv", "world"])
def test_shipped_decoders_train_through_the_kernel(golden, name):
    """B = 2, T = 4800, fixed noise, loss = (y * r).sum(); d loss / d {filter control track, log_mag, room kernel} of the
    routed decoder against the same decoder with hip_frames = False (the reference's arithmetic in fp32 on the device); then
    one backward under bf16 autocast with bf16 control tracks."""
    B, T = 2, 4800
    x = _inputs(name, B, T)
    dec = _decoder(golden, name, x)
    dec.noise_generator = _fixed_noise(x["noise"])
    stft = dec.harm_filter if name == "nhv" else dec.end_filter
    room = (dec.end_filter if name == "nhv" else dec.room_filter).kernel
    assert stft.hip_frames is True
    r = []   # the fixed random weights of the loss, drawn once the output length is known

    def grads(cast=lambda t: t):
        xs = dict(x)
        for k in ("ctrl", "log_mag"):
            xs[k] = cast(x[k]).detach().clone().requires_grad_()
        room.grad = None
        y = dec(noise_generator_params=(), **_call_args(name, xs)).as_tensor()
        if not r:
            r.append(torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).cuda())
        (y.float() * r[0]).sum().backward()
        return {"ctrl": xs["ctrl"].grad, "log_mag": xs["log_mag"].grad, "room": room.grad.clone()}

    routed = grads()
    stft.hip_frames = False
    try:
        stock = grads()
    finally:
        del stft.hip_frames
    for k in routed:
        assert torch.isfinite(routed[k]).all(), (name, k)
        emax, el2 = rel_err(_np(routed[k]), _np(stock[k]))
        print(f"{name} decoder d loss / d {k}: routed vs hip_frames = False rel-max {emax:.3e} L2 {el2:.3e}")
        assert emax <= BAR and el2 <= BAR, (name, k, emax, el2)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        low = grads(lambda t: t.to(torch.bfloat16))
    assert low["room"].dtype == torch.float32 and low["ctrl"].dtype == torch.bfloat16
    for k in low:
        assert torch.isfinite(low[k].float()).all(), (name, k)


def test_forward_and_backward_replay_in_a_graph():
    from golf_amd import functional as GF

    n, hop, T, F = 128, 32, 6 * 32 + 7, 9
    gen = torch.Generator().manual_seed(3)
    w = torch.hann_window(n).cuda()
    x = torch.randn(3, T, generator=gen).cuda().requires_grad_()
    H = _rows("complex", 3, F, n, gen).cuda().requires_grad_()
    gy = torch.randn(3, hop * 6, generator=gen).cuda()

    def step():
        return torch.autograd.grad(GF.stft_filter_frames(x, H, w, hop), (x, H), gy)

    ex, eH = step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                              # warm-up off the default stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gx, gH = step()
    for _ in range(2):
        gx.zero_(), gH.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gx, ex) and torch.equal(torch.view_as_real(gH), torch.view_as_real(eH))
