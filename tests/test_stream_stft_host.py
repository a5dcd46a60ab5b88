"""CPU: the bookkeeping of the streams built on the STFT-domain frame filter -- NHV (HarmonicPlusNoiseStream with an "stft"
branch) and WORLD (SpectralDecoderStream) -- as pure host functions of the pushed lengths, their refusals, and the argument
checks of golf_stft_filter_frames_stream_f32 (no launch)."""
import numpy as np
import pytest

# (n_fft, hop): hop not dividing n_fft, the golden fixtures' shape, the kernel's 64-lane block (the first size with one frame
# per block), its 128-lane block with a radix-2 last stage, the shipped one
STFT = [(64, 24), (128, 32), (256, 60), (512, 120), (1024, 240)]
FIR = dict(taps=510, hop=240)               # the noise filter of both shipped decoders (n_mag 256 at hop 240)


def shipped(golden, name):
    from golf_amd.config import build_model

    g = golden("g28_shipped_configs")
    m = build_model(str(g["config"][list(g["path"]).index(f"ckpts/interspeech24/{name}/config.yaml")]))
    return getattr(m, "decoder", m)


def geometry(name, n=1024, hop=240):
    """"nhv" / "world": the shipped decoders' geometry with the phase at hop 1; "stft": the filter alone on a pushed track."""
    from golf_amd.stream import BranchGeometry, HPNGeometry, SpectralGeometry

    b, fir = BranchGeometry("stft", hop=hop, window=n), BranchGeometry("fir", hop=FIR["hop"], taps=FIR["taps"])
    if name == "world":
        return SpectralGeometry(phase_hop=1, noise=fir, end=b)
    return HPNGeometry(phase_hop=1, harm=b, noise=fir if name == "nhv" else BranchGeometry())


def emit(g, n_phase, n_noise, n_fir, n_stft):
    from golf_amd.stream import SpectralGeometry, hpn_emit_count, spectral_emit_count

    if isinstance(g, SpectralGeometry):
        return spectral_emit_count(g, n_phase, None, n_noise, (n_fir,), (n_stft,))
    return hpn_emit_count(g, n_phase, None, n_noise, (n_stft,), (n_fir,) if g.noise.kind == "fir" else ())


def final(g, n_phase, n_noise, n_fir, n_stft):
    from golf_amd.stream import SpectralGeometry, hpn_final_lengths, spectral_final_lengths

    if isinstance(g, SpectralGeometry):
        return spectral_final_lengths(g, n_phase, None, n_noise, (n_fir,), (n_stft,))
    return hpn_final_lengths(g, n_phase, None, n_noise, (n_stft,), (n_fir,) if g.noise.kind == "fir" else ())


# ---- brute force: a sample is out once every frame that covers it is ready --------------------------------------------------
def _stft_ready(n, hop, n_in, rows):
    """Samples [0, E) all of whose covering frames f (0 <= m + n/2 - f*hop < n) have their response row and every sample they
    read: x[|i|] for i in [f*hop - n/2, f*hop + n/2) -- no right reflection while the input is open."""
    pad = n // 2
    reads = lambda f: max(abs(i) for i in (f * hop - pad, f * hop + pad - 1))
    m = 0
    while True:
        fs = [f for f in range(max(0, (m + pad - n) // hop), (m + pad) // hop + 1) if 0 <= m + pad - f * hop < n]
        if not all(f < rows and reads(f) < n_in for f in fs):
            return m
        m += 1


def _fir_ready(n_in, rows):
    """Whole frames: frame f reads its input up to (f+1)*hop - 1 + R, R = N-1-(N-1)//2."""
    hop, R = FIR["hop"], FIR["taps"] - 1 - (FIR["taps"] - 1) // 2
    f = 0
    while f < rows and (f + 1) * hop - 1 + R < n_in:
        f += 1
    return f * hop


def brute(name, n, hop, n_phase, n_noise, n_fir, n_stft):
    n_osc = max(0, n_phase - 1)          # the segment a phase step closes (phase at hop 1)
    nz_in = min(n_noise, n_phase)        # the noise the one-shot is certain to use
    if name == "stft":
        return min(_stft_ready(n, hop, n_osc, n_stft), nz_in)
    nz = _fir_ready(nz_in, n_fir)
    if name == "nhv":
        return min(_stft_ready(n, hop, n_osc, n_stft), nz)
    return _stft_ready(n, hop, min(n_osc, nz), n_stft)


@pytest.mark.parametrize("name,n,hop", [("stft", n, h) for n, h in STFT] + [("nhv", 1024, 240), ("world", 1024, 240)])
def test_emit_count_is_the_brute_force_count_and_monotone(name, n, hop):
    g = geometry(name, n, hop)
    rng = np.random.default_rng(n + hop + len(name))
    for trial in range(6):
        # (the decoders: long enough for the whole FIR frames of the noise branch to outlast WORLD's reflect pad)
        T = int(rng.integers(n // 2 + 1 if name == "stft" else 5 * hop, 14 * hop))
        F = max(2 if name == "stft" else 4, T // hop + int(rng.integers(-2, 4)))
        full = dict(phase=T, noise=T, fir=F, stft=F)
        fl = final(g, full["phase"], full["noise"], full["fir"], full["stft"])
        pos = dict.fromkeys(full, 0)
        last = 0
        while any(pos[k] < full[k] for k in full):
            for k in full:
                step = rng.choice([0, 1, 7, 17, hop, 333, 2400]) if k in ("phase", "noise") else rng.choice([0, 1, 2, 3])
                pos[k] = min(full[k], pos[k] + int(step))
            E = emit(g, pos["phase"], pos["noise"], pos["fir"], pos["stft"])
            assert E == brute(name, n, hop, pos["phase"], pos["noise"], pos["fir"], pos["stft"]), (name, pos, E)
            assert last <= E <= fl["out"], (name, pos, last, E, fl)
            last = E


@pytest.mark.parametrize("n,hop", STFT)
def test_final_lengths_are_the_modules_own(n, hop):
    """The lengths at finish against the shapes the modules' CPU forward returns: T just past the reflect pad, a multiple of
    hop and one either side of it, F below and above 1 + T // hop."""
    import torch

    from golf_amd._lib import GolfError
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import DiffWorldSPFilter, LTVCepFilter

    cep = LTVCepFilter(filter_order=8, n_fft=n, window="hanning", hop_length=hop, phase="min")
    world = DiffWorldSPFilter(n_mels=6, n_fft=n, hop_length=hop, f_min=0.0, f_max=4000.0, center=True, window="hanning",
                              sample_rate=8000, norm=None, mel_scale="htk")
    g = geometry("stft", n, hop)
    k = n // hop + 2
    for T in (n // 2 + 1, k * hop - 1, k * hop, k * hop + 1):
        for F in (max(1, T // hop - 1), T // hop + 1, T // hop + 4):
            x = AudioTensor(torch.randn(2, T))
            if min(1 + T // hop, F) < 2:   # a single frame: torch.istft has no sample to return and raises
                with pytest.raises(RuntimeError):
                    cep(x, AudioTensor(0.01 * torch.randn(2, F, 9), hop))
                with pytest.raises(GolfError, match=f"{T} input samples"):
                    final(g, T, T, 0, F)
                continue
            want = cep(x, AudioTensor(0.01 * torch.randn(2, F, 9), hop)).shape[1]
            assert world(x, AudioTensor(torch.rand(2, F, 6) + 0.1, hop)).shape[1] == want
            fl = final(g, T, T, 0, F)
            assert fl["out"] == want == hop * (min(1 + T // hop, F) - 1), (n, hop, T, F, fl, want)
            assert fl["harm"]["frames"] == min(1 + T // hop, F)


def test_an_utterance_the_reflect_pad_does_not_fit_is_refused():
    """T <= n_fft/2: torch.stft raises in the one-shot; the lengths at finish (and with them ``finish()``) raise GolfError."""
    import torch

    from golf_amd._lib import GolfError
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import LTVCepFilter

    cep = LTVCepFilter(filter_order=8, n_fft=64, window="hanning", hop_length=24, phase="zero")
    with pytest.raises(RuntimeError):
        cep(AudioTensor(torch.randn(1, 32)), AudioTensor(torch.zeros(1, 3, 9), 24))
    for name in ("stft", "nhv", "world"):
        with pytest.raises(GolfError, match="512"):
            final(geometry(name), 512, 512, 4, 4)
    assert final(geometry("stft"), 513, 513, 0, 9)["out"] == 480


def _first_time(E, t, lo, hi):
    if E(hi) <= t:
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if E(mid) > t:
            hi = mid
        else:
            lo = mid + 1
    return lo


@pytest.mark.parametrize("name,want", [("nhv", 1024), ("world", 1517)])
def test_latency_formula_is_a_bound_and_tight(name, want):
    """Every track pushed up to input time S: output t is out by S = t + latency at the latest, and some t needs more than
    latency - hop."""
    from golf_amd.stream import hpn_stream_latency, spectral_stream_latency

    g = geometry(name)
    L = (spectral_stream_latency if name == "world" else hpn_stream_latency)(g)
    assert L == want
    hop = 240
    E = lambda S: emit(g, S + 1, S + 1, S // hop + 1, S // hop + 1)
    worst = 0
    for t in range(0, 6 * hop + 1, 7):
        need = _first_time(E, t, t, t + L)
        assert need is not None, (name, t, L)
        worst = max(worst, need - t)
    assert L - hop < worst <= L, (name, worst, L)


def test_refusals(golden):
    import torch

    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import DiffWorldSPFilter, LTVCepFilter
    from golf_amd.noise import UniformNoise
    from golf_amd.stream import (DecoderStream, FramewiseDecoderStream, HarmonicPlusNoiseStream, SpectralDecoderStream,
                                 open_stream)
    from golf_amd.synth import PulseTrain
    from golf_amd.synthetic import make_decoder

    nhv, world = shipped(golden, "nhv"), shipped(golden, "world")
    assert type(open_stream(nhv, 2)) is HarmonicPlusNoiseStream and type(open_stream(world, 2)) is SpectralDecoderStream
    # the other classes keep refusing them, and the new class refuses theirs
    for cls, dec, what in ((DecoderStream, world, "AdditivePulseTrain"), (FramewiseDecoderStream, world, "AdditivePulseTrain"),
                           (FramewiseDecoderStream, nhv, "AdditivePulseTrain"), (SpectralDecoderStream, nhv, "HarmonicPlus"),
                           (SpectralDecoderStream, make_decoder(), "IndexedGlottalFlowTable")):
        with pytest.raises(NotImplementedError, match=what):
            cls(dec, 2)
    world_filter = lambda **kw: DiffWorldSPFilter(**{**dict(n_mels=80, n_fft=1024, hop_length=240, f_min=0.0, f_max=12000.0,
                                                           sample_rate=24000, norm=None, mel_scale="htk"), **kw})
    for build, what in ((lambda d: setattr(d, "end_filter", world_filter(center=False)), "center=False"),
                        (lambda d: setattr(d, "end_filter", world_filter(n_fft=960)), "n_fft 960"),
                        (lambda d: setattr(d, "end_filter", world_filter(n_fft=256)), "2\\*hop"),
                        (lambda d: setattr(d, "end_filter", world_filter(n_fft=4096)), "n_fft 4096"),
                        (lambda d: setattr(d, "subtract_harmonics", True), "subtract_harmonics"),
                        (lambda d: setattr(d, "noise_generator", UniformNoise()), "UniformNoise"),
                        (lambda d: setattr(d, "noise_filter", world_filter()), "noise filter"),
                        (lambda d: setattr(d, "room_filter", world_filter()), "room filter"),
                        (lambda d: setattr(d, "harm_oscillator", PulseTrain()), "PulseTrain")):
        d = shipped(golden, "world")
        build(d)
        with pytest.raises(NotImplementedError, match=what):
            SpectralDecoderStream(d, 2)
        with pytest.raises(NotImplementedError, match=what):
            open_stream(d, 2)
    d = shipped(golden, "nhv")
    d.harm_filter = LTVCepFilter(filter_order=240, n_fft=1000, window="hanning", hop_length=240, phase="min")
    with pytest.raises(NotImplementedError, match="n_fft 1000"):
        HarmonicPlusNoiseStream(d, 2)
    # push-time refusals (all before any device work)
    z = lambda *s, hop=1: AudioTensor(torch.zeros(*s), hop)
    st = SpectralDecoderStream(world, 2)
    args = dict(phase=z(2, 1), noise_filter_params=(z(2, 1, 256, hop=240),), end_filter_params=(z(2, 1, 80, hop=240),))
    with pytest.raises(NotImplementedError, match="voicing"):
        st.push(**args, voicing=z(2, 1))
    with pytest.raises(NotImplementedError, match="requires grad"):
        st.push(**{**args, "phase": AudioTensor(torch.zeros(2, 1, requires_grad=True))})
    with pytest.raises(NotImplementedError, match="initial_phase"):
        st.push(**args, harm_oscillator_params=(z(2, 155),))
    with pytest.raises(NotImplementedError, match="noise generator parameters"):
        st.push(**args, noise_generator_params=(z(2, 1),))
    with pytest.raises(ValueError, match="end_filter_params"):
        st.push(**{**args, "end_filter_params": ()})
    with pytest.raises(Exception, match="ROCm device"):   # CPU tensors: there is no CPU path
        st.push(**args)
    st = HarmonicPlusNoiseStream(nhv, 2)
    args = dict(phase=z(2, 1), noise_filter_params=(z(2, 1, 256, hop=240),), harm_filter_params=(z(2, 1, 241, hop=240),))
    with pytest.raises(ValueError, match="harm_filter_params must hold 1"):
        st.push(**{**args, "harm_filter_params": ()})
    with pytest.raises(ValueError, match="hop 120"):
        st.push(**{**args, "harm_filter_params": (z(2, 1, 241, hop=120),)})
    with pytest.raises(Exception, match="ROCm device"):
        st.push(**args)


def test_functional_entries_refuse_cpu_tensors():
    import torch

    from golf_amd import functional as GF
    from golf_amd._lib import GolfError

    x, H, w = torch.zeros(1, 200), torch.ones(1, 7, 33), torch.hann_window(64)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.stft_filter_frames(x, H, w, 24)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.stft_filter_stream(x, H.to(torch.complex64), w, 24, x0=0, h0=0, f0=0, nf=1, n0=0, ny=0)
    with pytest.raises(GolfError, match="reflect-padded"):
        GF.stft_filter_frames(x[:, :32], H, w, 24)


def test_stream_entry_refuses_bad_arguments_without_launch():
    import ctypes

    from golf_amd import _lib

    lib = _lib.load()
    sb = lib.golf_stft_filter_stream_state_bytes
    assert sb(2, 128, 32) == 4 * 2 * 3 * 128 and sb(1, 64, 24) == 4 * 2 * 64 and sb(1, 1024, 240) == 4 * 4 * 1024
    assert sb(1, 96, 32) == 0 and sb(1, 128, 65) == 0 and sb(0, 128, 32) == 0 and sb(1, 4096, 240) == 0 and sb(1, 32, 8) == 0
    f = lib.golf_stft_filter_frames_stream_f32
    one = ctypes.c_void_p(256)   # never dereferenced: every call below is refused on its arguments
    # a valid first call: frames 0..3 of n_fft 128 / hop 32 read samples [0, 160) and response rows 0..3, write samples [0, 64)
    ok = dict(x=one, x_stride=160, x0=0, nx=160, x_end=-1, h=one, h0=0, nh=4, h_kind=1, frames_end=-1, window=one, f0=0, nf=4,
              y=one, y_stride=64, n0=0, ny=64, B=2, n_fft=128, hop=32, carry=one, ws=one, ws_bytes=1 << 40, stream=None)
    names = list(ok)

    def refused(match, code=-1, **kw):
        rc = f(*[kw.get(k, ok[k]) for k in names])
        assert rc == code, (kw, rc, lib.golf_last_error())
        assert match.encode() in lib.golf_last_error(), (kw, lib.golf_last_error())

    for k in ("carry", "window", "x", "h", "ws", "y"):
        refused("null", **{k: None})
    refused("power of two", code=-3, n_fft=96)
    refused("power of two", code=-3, n_fft=4096)
    refused("power of two", code=-3, n_fft=32, hop=8)
    refused("< 2*hop", hop=65)
    refused("bad size", f0=-1)
    refused("bad size", h_kind=2)
    refused("both open", x_end=5000)
    refused("both open", frames_end=6)
    refused("input window", nx=159)
    refused("input window", x0=1)
    refused("response window", nh=3)
    refused("response window", h0=1)
    refused("not filtered yet", ny=65, y_stride=65)
    refused("stride", y_stride=10)
    refused("stride", x_stride=100)
    refused("workspace", code=-2, ws_bytes=4 * 2 * 7 * 128 - 1)
    refused("written without frame", f0=4, nf=1, n0=96, ny=0, x0=64, nx=128, h0=4, nh=1)   # frame 4 reaches sample 64
    refused("write the samples", ny=32)                                  # samples 32.. would lose frame 0
    refused("carry holds", f0=8, nf=0, n0=32, ny=32)                     # frame 0 is long gone
    # once the utterance has ended: T > n_fft/2, frames <= 1 + T // hop, frames and samples within them
    refused("reflect-padded", x_end=64, frames_end=1)
    refused("frames_end", x_end=160, frames_end=7)
    refused("frames past the last", x_end=160, frames_end=3)
    refused("samples past the end", x_end=160, frames_end=4, ny=97, y_stride=97)
    # T = 5 * hop: the last frame (5) spans [96, 224) and its reflection reads down to x[2*159 - 223] = x[95]
    last = dict(x_end=160, frames_end=6, f0=5, nf=1, h0=5, nh=1, n0=96, ny=64)
    refused("input window does not cover samples [95", x0=96, nx=64, **last)
    refused("workspace", code=-2, x0=95, nx=65, ws_bytes=0, **last)      # (the window from x[95] on passes that check)
    # nothing to do is not an error, and touches no pointer
    assert f(*[dict(ok, nf=0, ny=0, ws=None, ws_bytes=0, x=None, h=None, y=None)[k] for k in names]) == 0
