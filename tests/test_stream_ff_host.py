"""CPU: the frame-wise streaming decoders' bookkeeping (golf-ff and golf-v1: pure host functions of the pushed lengths,
checked against the float64 oracle composition), their refusals and dispatch, and the argument checks of the streaming
frame-wise filter entry (no launch)."""
import numpy as np
import pytest

GSS = dict(hop=240, phase_hop=1, os=4, half=64, w_hop=2400, fir_taps=510, fir_hop=240)
GFF = dict(GSS, window=960)
GV1 = dict(GSS, window=960, hpn=True)


def geometry(**kw):
    from golf_amd.stream import StreamGeometry

    return StreamGeometry(**kw)


def _compose(inp, table, taps, hpn):
    """The one-shot decoder as the float64 oracle composes it (tests/test_config.py): golf-ff or golf-v1."""
    import torch

    from oracle import golf_oracle as O

    src = O.indexed_glottal_forward(inp["phase"], 1, inp["wsel"], inp["w_hop"], table, 4, True, decim_taps=taps)["out"]
    kern = O.zero_phase_fir_kernels(inp["log_mag"], torch.hann_window(510, dtype=torch.float64).numpy())
    nz = O.ltv_fir_frames_forward(inp["noise"][:, : src.shape[1]], kern, 240)
    win = torch.hann_window(960, dtype=torch.float64).numpy()
    if hpn:
        harm = O.lti_frames_ola_forward(src, inp["gain"], inp["a"], 240, win)[0]
        n = min(harm.shape[1], nz.shape[1])
        y = harm[:, :n] + nz[:, :n]
    else:
        n = min(src.shape[1], nz.shape[1])
        y = O.lti_frames_ola_forward(src[:, :n] + nz[:, :n], inp["gain"], inp["a"], 240, win)[0]
    return O.lti_acoustic_filter_forward(y, inp["room_kernel"])


@pytest.mark.parametrize("hpn", [False, True], ids=["golf-ff", "golf-v1"])
def test_emitted_samples_depend_only_on_pushed_inputs(hpn):
    """For random push prefixes, every input step not yet pushed is replaced by other values (lengths kept): the first
    emit_count(...) samples of the oracle composition do not move, and the final length is the composition's."""
    from golf_amd.stream import emit_count, final_lengths
    from golf_amd.synthetic import make_decoder, make_inputs

    g = geometry(**(GV1 if hpn else GFF))
    T = 7200
    c = lambda d: {k: (v.double().numpy() if hasattr(v, "numpy") else v) for k, v in d.items()}
    base = c(make_inputs(B=1, T=T, with_noise_filter=True))
    other = c(make_inputs(B=1, T=T, with_noise_filter=True, seed=7))
    osc = make_decoder(framewise=True).harm_oscillator
    table, taps = osc.table.double().numpy(), osc.decimater.taps.double().numpy()
    ref = _compose(base, table, taps, hpn)
    F = base["a"].shape[1]
    assert final_lengths(g, T, T, F, F)["out"] == ref.shape[1]
    rng = np.random.default_rng(21 + hpn)
    keys = ("phase", "wsel", "noise", "log_mag", "gain", "a")
    checked = 0
    for _ in range(8):
        n = {k: int(rng.integers(0, base[k].shape[1] + 1)) for k in keys}
        if rng.random() < 0.5:   # everything up to one input time, the way a live stream pushes
            S = int(rng.integers(0, T))
            n = dict(phase=S + 1, wsel=S // 2400 + 1, noise=S + 1, log_mag=S // 240 + 1, gain=S // 240 + 1, a=S // 240 + 1)
            n = {k: min(v, base[k].shape[1]) for k, v in n.items()}
        E = emit_count(g, n["phase"], n["wsel"], n["noise"], n["log_mag"], n["gain"], n["a"])
        mod = dict(base)
        for k in keys:
            mod[k] = np.concatenate([base[k][:, : n[k]], other[k][:, n[k]:]], 1)
        y = _compose(mod, table, taps, hpn)
        assert y.shape == ref.shape
        if E:
            err = np.abs(y[:, :E] - ref[:, :E]).max() / np.abs(ref).max()
            assert err <= 1e-12, (n, E, err)
            checked += 1
        # and the sample after E does depend on something not pushed (E is not needlessly small) for a full-time prefix
    assert checked >= 2


def _first_time(E, t, lo, hi):
    """Smallest s in [lo, hi] with E(s) > t (E non-decreasing), or None."""
    if E(hi) <= t:
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if E(mid) > t:
            hi = mid
        else:
            lo = mid + 1
    return lo


@pytest.mark.parametrize("kw", [GFF, GV1, dict(GFF, fir_taps=0), dict(GV1, phase_hop=240, w_hop=480),
                                dict(GFF, window=480, hop=240), dict(GV1, window=1000, hop=250, fir_hop=250, w_hop=2500)],
                         ids=["golf-ff", "golf-v1", "ff-no-fir", "v1-coarse-phase", "ff-W2hop", "v1-hop250"])
def test_latency_formula_is_a_bound_and_tight(kw):
    from golf_amd.stream import emit_count, stream_latency

    g = geometry(**kw)
    L = stream_latency(g)

    def E(S):  # every track pushed up to input time S
        return emit_count(g, S // g.phase_hop + 1, S // g.w_hop + 1, S + 1, S // g.fir_hop + 1, S // g.hop + 1,
                          S // g.hop + 1)

    worst = 0
    for t in range(0, 3 * max(g.w_hop, g.hop, g.phase_hop) * 4):
        need = _first_time(E, t, t, t + L)
        assert need is not None, (kw, t)
        worst = max(worst, need - t)
    assert worst <= L, (kw, worst, L)
    if kw is GFF or kw is GV1:   # the shipped geometries: within one LPC hop of the worst case actually met
        assert L - g.hop < worst, (worst, L)
        assert L == 3375


def test_final_lengths_match_the_one_shot_modules():
    from golf_amd import functional as GF
    from golf_amd.stream import final_lengths

    for T in (4800, 7199, 7200, 7201, 12345, 48000):
        osc = GF.osc_lengths(T, 1, 4)[1]
        for F in (T // 240 - 3, T // 240, T // 240 + 1, T // 240 + 5):
            for n_noise in (None, T - 500):
                noise = osc if n_noise is None else min(n_noise, osc)
                nz = GF.fir_frames_length(noise, F, 510, 240)
                Ty_ff = GF.ff_output_length(min(osc, nz), F, 240, 960)
                Ty_v1 = GF.ff_output_length(osc, F, 240, 960)
                if Ty_ff[1] <= F:
                    fl = final_lengths(geometry(**GFF), T, n_noise, F, F)
                    assert fl["out"] == Ty_ff[2] and fl["frames"] == Ty_ff[1] and fl["filter_in"] == Ty_ff[0], (T, F)
                if Ty_v1[1] <= F:
                    fl = final_lengths(geometry(**GV1), T, n_noise, F, F)
                    assert fl["filter_out"] == Ty_v1[2] and fl["noise_filter"] == nz
                    assert fl["out"] == min(Ty_v1[2], nz), (T, F)
    # without a noise filter, golf-ff's source is the oscillator itself
    fl = final_lengths(geometry(**dict(GFF, fir_taps=0)), 48000, None, 0, 200)
    assert fl["out"] == GF.ff_output_length(48000, 200, 240, 960)[2] == 47760
    # the golf-ss geometry (no frame window) keeps its old lengths and latency
    assert final_lengths(geometry(**GSS), 48000, None, 200, 200)["out"] == 47760
    from golf_amd.stream import stream_latency

    assert stream_latency(geometry(**GSS)) == 2655


def _v1(golden, rel="ckpts/interspeech24/golf-v1/config.yaml"):
    from golf_amd.config import build_model

    g = golden("g28_shipped_configs")
    paths = list(g["path"])
    return getattr(build_model(str(g["config"][paths.index(rel)])), "decoder")


def test_refusals_and_dispatch(golden):
    import torch

    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import LTVZeroPhaseFIRFilterPrecise
    from golf_amd.noise import UniformNoise
    from golf_amd.sf import HarmonicPlusNoiseSynth
    from golf_amd.stream import DecoderStream, FramewiseDecoderStream, open_stream
    from golf_amd.synthetic import make_ddsp_decoder, make_decoder

    v1 = _v1(golden)
    assert isinstance(v1, HarmonicPlusNoiseSynth)
    assert type(open_stream(make_decoder(framewise=True), 2)) is FramewiseDecoderStream
    assert type(open_stream(v1, 2)) is FramewiseDecoderStream
    assert type(open_stream(make_decoder(), 2)) is DecoderStream
    # DecoderStream keeps refusing both
    with pytest.raises(NotImplementedError, match="LTVMinimumPhaseFilter"):
        DecoderStream(make_decoder(framewise=True), 2)
    with pytest.raises(NotImplementedError, match="HarmonicPlusNoiseSynth"):
        DecoderStream(v1, 2)
    # and the frame-wise stream refuses what it does not cover
    with pytest.raises(NotImplementedError, match="AdditiveSynthesizer"):
        FramewiseDecoderStream(make_ddsp_decoder(), 2)
    with pytest.raises(NotImplementedError, match="AdditiveSynthesizer"):
        open_stream(make_ddsp_decoder(), 2)
    with pytest.raises(NotImplementedError, match="LTVMinimumPhaseFilterPrecise"):
        FramewiseDecoderStream(make_decoder(), 2)
    d = make_decoder(framewise=True)
    d.end_filter.centred = False
    with pytest.raises(NotImplementedError, match="centred=False"):
        FramewiseDecoderStream(d, 2)
    d = _v1(golden)
    d.harm_filter.centred = False
    with pytest.raises(NotImplementedError, match="centred=False"):
        FramewiseDecoderStream(d, 2)
    d = make_decoder(framewise=True)
    d.noise_generator = UniformNoise()
    with pytest.raises(NotImplementedError, match="UniformNoise"):
        FramewiseDecoderStream(d, 2)
    d = _v1(golden)
    d.noise_generator = UniformNoise()
    with pytest.raises(NotImplementedError, match="UniformNoise"):
        FramewiseDecoderStream(d, 2)
    d = make_decoder(framewise=True)
    d.noise_filter = LTVZeroPhaseFIRFilterPrecise(window="hanning", n_mag=256)
    with pytest.raises(NotImplementedError, match="LTVZeroPhaseFIRFilterPrecise"):
        FramewiseDecoderStream(d, 2)
    d = make_decoder(framewise=True)
    d.subtract_harmonics = True
    with pytest.raises(NotImplementedError, match="subtract_harmonics"):
        FramewiseDecoderStream(d, 2)
    z = lambda *s: AudioTensor(torch.zeros(*s))
    lpc = (AudioTensor(torch.zeros(2, 1), 240), AudioTensor(torch.zeros(2, 1, 22), 240))
    base = dict(phase=z(2, 1), harm_oscillator_params=(AudioTensor(torch.zeros(2, 1), 2400),),
                noise_filter_params=(AudioTensor(torch.zeros(2, 1, 256), 240),))
    for dec, key in ((make_decoder(framewise=True), "end_filter_params"), (_v1(golden), "harm_filter_params")):
        st = FramewiseDecoderStream(dec, 2)
        args = {**base, key: lpc}
        with pytest.raises(NotImplementedError, match="voicing"):
            st.push(**args, voicing=z(2, 1))
        g = AudioTensor(torch.zeros(2, 1, requires_grad=True), 240)
        with pytest.raises(NotImplementedError, match="requires grad"):
            st.push(**{**args, key: (g, lpc[1])})
        other = "harm_filter_params" if key == "end_filter_params" else "end_filter_params"
        with pytest.raises(ValueError, match=key):
            st.push(**{**base, other: lpc})
        with pytest.raises(Exception, match="ROCm device"):   # CPU tensors: there is no CPU path
            st.push(**args)


def test_stream_entry_refuses_bad_arguments_without_launch():
    import ctypes

    from golf_amd import _lib

    lib = _lib.load()
    sb = lib.golf_lti_frames_stream_state_bytes
    assert sb(2, 960, 240, 22) == 4 * 2 * 3 * 960
    assert sb(1, 1000, 250, 7) == 4 * 3 * 1000 and sb(1, 480, 240, 22) == 4 * 480
    assert sb(1, 959, 480, 22) == 0 and sb(1, 960, 240, 39) == 0 and sb(0, 960, 240, 22) == 0
    f = lib.golf_lti_frames_ola_stream_f32
    one = ctypes.c_void_p(256)   # never dereferenced: every call below is refused on its arguments
    big = 1 << 40
    # a valid first call: frames 0..3 of W 960 / hop 240 read samples [0, 1200) and gain rows 0..5, write samples [0, 480)
    ok = dict(ex=one, ex_stride=1200, x0=0, nx=1200, x_end=-1, gain=one, g0=0, ng=6, g_end=-1, a=one, a0=0, na=4,
              window=one, f0=0, nf=4, y=one, y_stride=480, n0=0, ny=480, B=2, M=22, hop=240, W=960, carry=one, ws=one,
              ws_bytes=big, stream=None)
    names = list(ok)

    def call(**kw):
        return f(*[kw.get(k, ok[k]) for k in names])

    def refused(match, code=-1, **kw):
        rc = call(**kw)
        assert rc == code, (kw, rc, lib.golf_last_error())
        assert match.encode() in lib.golf_last_error(), (kw, lib.golf_last_error())

    refused("null", carry=None)
    refused("null", window=None)
    refused("null", ex=None)
    refused("null", ws=None)
    refused("null", y=None)
    refused("window 400 < 2*hop", W=400)
    refused("M <= 38", code=-3, M=39)
    refused("negative", f0=-1)
    refused("both open", x_end=5000)
    refused("excitation window", nx=1199)
    refused("excitation window", x0=1)
    refused("gain window", ng=5)
    refused("a window", na=3)
    refused("a window", a0=1, na=4)
    refused("not filtered yet", ny=481, y_stride=481)
    refused("stride", y_stride=100)
    refused("stride", ex_stride=1000)
    refused("workspace", code=-2, ws_bytes=4 * 2 * 7 * 960 - 1)
    refused("written without frame", f0=4, nf=1, n0=720, ny=0, x0=240, g0=2, a0=4, na=1)   # frame 4 reaches sample 480
    refused("write the samples", ny=240)                                            # samples 240.. would lose frame 0
    refused("carry holds", f0=8, nf=0, n0=240, ny=240)                              # frame 0 is long gone
    # once the utterance has ended: x_end <= (g_end-1)*hop+1, frames and samples within nfr and Ty
    refused("exceeds", x_end=1202, g_end=6)
    refused("frames past the last", x_end=700, g_end=6)                             # nfr = 3
    refused("samples past the end", x_end=960, g_end=6, nf=5, na=5, ny=961, y_stride=961)
    refused("both open", x_end=-1, g_end=6)
    # nothing to do is not an error, and touches no pointer
    assert f(*[dict(ok, nf=0, ny=0, ws=None, ws_bytes=0, ex=None, gain=None, a=None, y=None)[k] for k in names]) == 0
