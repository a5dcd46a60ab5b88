"""The STFT-domain frame filter on the device: golf_stft_filter_frames_stream_f32 against the reference's own runs, bit for bit
under random splits into calls and against the modules' float64 CPU forward; the NHV and WORLD decoders streamed
(HarmonicPlusNoiseStream, SpectralDecoderStream) against the one-shot decoders and a float64 composition; bf16 autocast.

Bounds: the streaming contract of INTEGRATION.md -- <= 2e-4 rel-max from the one-shot decoder, <= 1e-4 (rel-max and L2) from
the float64 evaluation.  Every test prints the measured distances of the kernel and of torch's fp32 one-shot."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from test_stream_stft_host import STFT, shipped

pytestmark = pytest.mark.gpu


def _cep(n, hop, phase="min", order=24):
    from golf_amd.filters import LTVCepFilter

    return LTVCepFilter(filter_order=order, n_fft=n, window="hanning", hop_length=hop, phase=phase)


def _world(n, hop, n_mels=12):
    from golf_amd.filters import DiffWorldSPFilter

    return DiffWorldSPFilter(n_mels=n_mels, n_fft=n, hop_length=hop, f_min=0.0, f_max=4000.0, center=True, window="hanning",
                             sample_rate=8000, norm=None, mel_scale="htk")


def _response(flt, ctrl):
    """(B, F, n/2+1) response rows as the module forms them (the stream's own code path)."""
    from golf_amd.stream import BranchGeometry, _BranchStage, _Track

    st = _BranchStage(BranchGeometry("stft", hop=flt.hop_length, window=flt.n_fft), flt, _Track(), ctrl.shape[0], ctrl.device)
    return st._response(ctrl)


def _forward64(flt, x, ctrl):
    """The module's own forward in float64 on the CPU."""
    import copy

    from golf_amd.audiotensor import AudioTensor as AT

    f64 = copy.deepcopy(flt).cpu().double()
    return f64(AT(x.double().cpu()), AT(ctrl.double().cpu(), flt.hop_length)).as_tensor().numpy()


def _report(what, got, one, ref):
    k, o = rel_err(got.cpu().numpy(), ref), rel_err(one.cpu().numpy(), ref)
    print(f"{what}: kernel vs float64 rel-max {k[0]:.3e} L2 {k[1]:.3e}; torch fp32 one-shot vs float64 {o[0]:.3e} {o[1]:.3e}")
    return k


@pytest.mark.parametrize("case", ["zero", "min", "world"])
def test_frames_match_the_references_own_runs(golden, case):
    from golf_amd import functional as GF
    from golf_amd.audiotensor import AudioTensor as AT

    if case == "world":
        g = golden("g22_world_sp_filter")
        flt = _world(128, 32).cuda()
        x, ctrl, want = torch.from_numpy(g["ex"]).float().cuda(), torch.exp(torch.from_numpy(g["logmel"]).float()).cuda(), g["y"]
    else:
        g = golden("g21_cep_filter")
        flt = _cep(128, 32, case).cuda()
        x, ctrl, want = (torch.from_numpy(g[f"{case}_ex"]).float().cuda(), torch.from_numpy(g[f"{case}_ceps"]).float().cuda(),
                         g[f"{case}_y"])
    H = _response(flt, ctrl)
    assert H.is_complex() == (case == "min")
    y = GF.stft_filter_frames(x, H, flt._window, 32)
    assert y.shape == want.shape and y.dtype == torch.float32
    one = flt(AT(x), AT(ctrl, 32)).as_tensor()
    emax, el2 = _report(f"reference run ({case})", y, one, want)
    assert emax <= 1e-4 and el2 <= 1e-4, (emax, el2)


def _split_calls(x, H, window, hop, rng):
    """Drive the entry as a stream does: samples and response rows arrive in independent random slices; each call filters
    the frames that are ready and writes the samples they finish, given only the samples from one before the next frame's
    start on; the last call runs with the end markers set."""
    from golf_amd import functional as GF

    B, T = x.shape
    F, n = H.shape[1], window.numel()
    pad = n // 2
    frames = min(1 + T // hop, F)
    carry, outs = None, []
    n_x = n_h = f0 = n0 = x_lo = calls = 0
    while n_x < T or n_h < F:
        n_x = min(T, n_x + int(rng.choice([0, 1, 7, hop, hop + 3, 2 * hop])))
        n_h = min(F, n_h + int(rng.choice([0, 1, 2])))
        nfr = min(n_h, (n_x - pad) // hop + 1) if n_x > pad else 0   # (frame 0 reads x[pad] through its left reflection)
        n_y = max(0, nfr * hop - pad)
        if nfr > f0 or n_y > n0:
            y, carry = GF.stft_filter_stream(x[:, x_lo:n_x], H[:, f0:n_h], window, hop, carry, x0=x_lo, h0=f0, f0=f0,
                                             nf=nfr - f0, n0=n0, ny=n_y - n0)
            outs.append(y)
            f0, n0, calls = nfr, n_y, calls + 1
            x_lo = max(0, f0 * hop - pad - 1)
    y, carry = GF.stft_filter_stream(x[:, x_lo:], H[:, f0:], window, hop, carry, x0=x_lo, h0=f0, f0=f0, nf=frames - f0, n0=n0,
                                     ny=hop * (frames - 1) - n0, x_end=T, frames_end=frames)
    outs.append(y)
    return torch.cat(outs, 1), calls + 1


@pytest.mark.parametrize("n,hop", STFT)
def test_entry_is_bitwise_independent_of_the_split(n, hop):
    """B = 3; T = 5 hop + 7 and T = 6 hop exactly (the last frame's reflection reads one sample before its own span); F on
    both sides of 1 + T // hop; the cepstral filter (complex rows) and the WORLD gain (real rows)."""
    from golf_amd import functional as GF
    from golf_amd.audiotensor import AudioTensor as AT

    gen = torch.Generator().manual_seed(n + hop)
    rng = np.random.default_rng(n)
    for kind, flt in (("cep", _cep(n, hop, order=min(24, n // 2 - 1)).cuda()), ("world", _world(n, hop).cuda())):
        for T in (5 * hop + 7, 6 * hop):
            for F in (T // hop, T // hop + 3):
                x = torch.randn(3, T, generator=gen).cuda()
                if kind == "cep":
                    ctrl = (torch.randn(3, F, flt.filter_order + 1, generator=gen) * 0.2 / (1 + torch.arange(flt.filter_order + 1))).cuda()
                else:
                    ctrl = torch.exp(0.3 * torch.randn(3, F, 12, generator=gen) - 2).cuda()
                H = _response(flt, ctrl)
                single = GF.stft_filter_frames(x, H, flt._window, hop)
                split, calls = _split_calls(x, H, flt._window, hop, rng)
                assert calls >= 3 and single.shape == split.shape == (3, hop * (min(1 + T // hop, F) - 1))
                assert torch.equal(single, split), (kind, n, hop, T, F, (single - split).abs().max())
                ref = _forward64(flt, x, ctrl)
                one = flt(AT(x), AT(ctrl, hop)).as_tensor()
                emax, el2 = _report(f"{kind} n {n} hop {hop} T {T} F {F}", single, one, ref)
                assert emax <= 1e-4 and el2 <= 1e-4, (kind, n, hop, T, F, emax, el2)


def test_one_frame_calls_wrap_the_ring():
    """B 2, n_fft 64, hop 16 (S = 3), T = 10 hop: one frame per call from frame 0 to frame 8 (the last two reach beyond T and
    wait for the end), so the slots the carried frames are read from and written to wrap more than once; the bits of the
    single call."""
    from golf_amd import functional as GF

    B, n, hop = 2, 64, 16
    T, pad = 10 * hop, n // 2
    frames = 1 + T // hop
    gen = torch.Generator().manual_seed(6416)
    x = torch.randn(B, T, generator=gen).cuda()
    H = torch.complex(torch.rand(B, frames, pad + 1, generator=gen) + 0.5, 0.2 * torch.randn(B, frames, pad + 1, generator=gen)).cuda()
    window = torch.hann_window(n).cuda()
    single = GF.stft_filter_frames(x, H, window, hop)
    carry, outs, n0 = None, [], 0
    for f in range(frames - 1):
        last = f == frames - 2
        x_lo = max(0, f * hop - pad - 1)
        n1 = hop * (frames - 1) if last else max(0, (f + 1) * hop - pad)
        y, carry = GF.stft_filter_stream(x[:, x_lo:T if last else f * hop + pad + 1], H[:, f:f + 1 + last], window, hop, carry,
                                         x0=x_lo, h0=f, f0=f, nf=1 + last, n0=n0, ny=n1 - n0, x_end=T if last else -1,
                                         frames_end=frames if last else -1)
        outs.append(y)
        n0 = n1
    split = torch.cat(outs, 1)
    assert single.shape == split.shape == (B, hop * (frames - 1)) and single.abs().max() > 0.1
    assert torch.equal(single, split), (single - split).abs().max()


# ---- the decoders --------------------------------------------------------------------------------------------------------
def _inputs(name, B, T, seed=2434):
    from golf_amd.synthetic import make_inputs

    base = make_inputs(B=B, T=T, hop=240, seed=seed, with_noise_filter=True, device="cuda")
    F = base["gain"].shape[1]
    gen = torch.Generator().manual_seed(seed)
    if name == "nhv":
        ctrl = (torch.randn(B, F, 241, generator=gen) * 0.05 / (1 + torch.arange(241))).cuda()
    else:
        ctrl = torch.exp(0.3 * torch.randn(B, F, 80, generator=gen) - 2).cuda()
    return dict(phase=base["phase"], noise=base["noise"], log_mag=base["log_mag"], ctrl=ctrl, room_kernel=base["room_kernel"])


def _call_args(name, x, cast=lambda t: t):
    from golf_amd.audiotensor import AudioTensor as AT

    key = "harm_filter_params" if name == "nhv" else "end_filter_params"
    return {"phase": AT(x["phase"]), "harm_oscillator_params": (), "noise_filter_params": (AT(cast(x["log_mag"]), 240),),
            key: (AT(cast(x["ctrl"]), 240),)}


def _fixed_noise(noise):
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.noise import NoiseInterface

    class Fixed(NoiseInterface):
        uses_reference_values = False

        def forward(self, ref, *args, **kwargs):
            return AudioTensor(noise[:, : ref.shape[1]])

    return Fixed()


def _decoder(golden, name, x):
    dec = shipped(golden, name).cuda().eval()
    with torch.no_grad():
        (dec.end_filter if name == "nhv" else dec.room_filter).kernel.copy_(x["room_kernel"])
    return dec


def _push_random(st, name, x, rng, noise=True, cast=lambda t: t):
    from golf_amd.audiotensor import AudioTensor as AT

    tracks = [("phase", 1), ("log_mag", 240), ("ctrl", 240)] + ([("noise", 1)] if noise else [])
    pos = dict.fromkeys([k for k, _ in tracks], 0)
    choice = lambda hop: [0, 1, 7, 17, 240, 333, 2400, 4801] if hop == 1 else [0, 1, 2, 3, 11]
    outs = []
    while any(pos[k] < x[k].shape[1] for k, _ in tracks):
        sl = {}
        for k, hop in tracks:
            m = int(rng.choice(choice(hop)))
            sl[k] = x[k][:, pos[k]: pos[k] + m]
            pos[k] = min(pos[k] + m, x[k].shape[1])
        outs.append(st.push(**_call_args(name, sl, cast), noise=AT(sl["noise"]) if noise else None))
    outs.append(st.finish())
    return torch.cat(outs, 1)


def _compose64(name, dec, x, nb):
    """The one-shot decoder in float64: the oracle's oscillator, zero-phase FIR and room filter, and the STFT-domain filter
    module's own forward in float64 on the CPU."""
    from oracle import golf_oracle as O

    c = lambda t: t[:nb].double().cpu().numpy()
    ph = c(x["phase"])
    sc = 1.0 / np.sqrt(0.5 / ph)
    src = O.harmonic_oscillator_forward(ph, 1, np.repeat(sc[:, :, None], dec.harm_oscillator.num_harmonics, 2), 1)
    win = dec.noise_filter._window(510, "cpu").double().numpy()
    nz = O.ltv_fir_frames_forward(c(x["noise"])[:, : src.shape[1]], O.zero_phase_fir_kernels(c(x["log_mag"]), win), 240)
    stft = lambda f, v: _forward64(f, torch.from_numpy(v), x["ctrl"][:nb])
    if name == "nhv":
        yh = stft(dec.harm_filter, src)
        m = min(yh.shape[1], nz.shape[1])
        y = yh[:, :m] + nz[:, :m]
    else:
        m = min(src.shape[1], nz.shape[1])
        y = stft(dec.end_filter, src[:, :m] + nz[:, :m])
    return O.lti_acoustic_filter_forward(y, x["room_kernel"].double().cpu().numpy())


@pytest.mark.parametrize("name", ["nhv", "world"])
def test_decoder_stream_vs_one_shot_and_float64(golden, name):
    from golf_amd.stream import HarmonicPlusNoiseStream, SpectralDecoderStream, open_stream

    B, T = 4, 7200
    x = _inputs(name, B, T)
    dec = _decoder(golden, name, x)
    dec.noise_generator = _fixed_noise(x["noise"])
    with torch.no_grad():
        one = dec(noise_generator_params=(), **_call_args(name, x)).as_tensor()
    st = open_stream(dec, B)
    assert type(st) is (HarmonicPlusNoiseStream if name == "nhv" else SpectralDecoderStream)
    y = _push_random(st, name, x, np.random.default_rng(3))
    assert st.latency == (1024 if name == "nhv" else 1517)
    assert y.shape == one.shape and y.shape[1] >= T - 480, (y.shape, one.shape)
    emax, _ = rel_err(y.cpu().numpy(), one.cpu().numpy())
    print(name, "stream vs one-shot decoder rel-max", emax)
    assert emax <= 2e-4, emax
    nb = 2
    ref = _compose64(name, dec, x, nb)
    emax, el2 = _report(f"{name} decoder", y[:nb], one[:nb], ref)
    assert emax <= 1e-4 and el2 <= 1e-4, (emax, el2)
    y2 = _push_random(open_stream(dec, B), name, x, np.random.default_rng(4))
    assert torch.equal(y, y2)


def test_nhv_generated_noise_and_autocast_bf16(golden):
    """NHV drawing its own noise, under bf16 autocast with bf16 control tracks, against fp32 streaming of the same values and
    noise (the bound of the existing autocast tests)."""
    from golf_amd.stream import HarmonicPlusNoiseStream

    x = _inputs("nhv", 2, 7200)
    dec = _decoder(golden, "nhv", x)
    bf = lambda t: t.to(torch.bfloat16)
    torch.manual_seed(0)
    y32 = _push_random(HarmonicPlusNoiseStream(dec, 2), "nhv", x, np.random.default_rng(1), noise=False,
                       cast=lambda t: bf(t).float())
    torch.manual_seed(0)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y16 = _push_random(HarmonicPlusNoiseStream(dec, 2), "nhv", x, np.random.default_rng(1), noise=False, cast=bf)
    assert y16.dtype == torch.float32 and y16.shape == y32.shape
    assert torch.isfinite(y16).all()
    _, el2 = rel_err(y16.cpu().numpy(), y32.cpu().numpy())
    print("nhv bf16 autocast vs fp32 on bf16-rounded inputs, L2", el2)
    assert el2 < 5e-2, el2


@pytest.mark.parametrize("name", ["nhv", "world"])
def test_finish_refuses_an_utterance_shorter_than_the_reflect_pad(golden, name):
    from golf_amd._lib import GolfError
    from golf_amd.stream import open_stream

    x = _inputs(name, 2, 7200)
    dec = _decoder(golden, name, x)
    short = {k: (v[:, :500] if k in ("phase", "noise") else v[:, :3]) for k, v in x.items() if k != "room_kernel"}
    st = open_stream(dec, 2)
    assert st.push(**_call_args(name, short)).shape == (2, 0)
    with pytest.raises(GolfError, match="cannot be reflect-padded"):
        st.finish()
