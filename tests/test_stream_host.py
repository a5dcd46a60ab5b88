"""CPU: the streaming decoder's block bookkeeping (pure host functions of the pushed lengths), its refusals, and the argument
checks of the streaming C entries (no launch)."""
import pytest

GSS = dict(hop=240, phase_hop=1, os=4, half=64, w_hop=2400, fir_taps=510, fir_hop=240)


def geometry(**kw):
    from golf_amd.stream import StreamGeometry

    return StreamGeometry(**{**GSS, **kw})


def test_emit_count_hand_worked():
    from golf_amd.stream import emit_count

    g = geometry()
    E = lambda ph, w, nz, lm, ga: emit_count(g, ph, w, nz, lm, ga, ga)
    assert E(0, 0, None, 0, 0) == 0
    assert E(1, 1, None, 1, 1) == 0                       # one sample of everything: no segment is closed
    # phase, noise and frames to t = 4800, two table-select rows (0, 1: fine samples < 9600 renderable): the oscillator's
    # outputs o with 4o + 64 <= 9599 are 2384 -> 9 whole frames
    assert E(4801, 2, None, 21, 21) == 2160
    # a third row: now the noise filter bounds it, frames f with (f+1)*240 + 255 <= 4801 -> 18 frames
    assert E(4801, 3, None, 21, 21) == 4320
    # gain / a: frame E/hop must be there to close the last frame
    assert E(4801, 3, None, 21, 10) == 9 * 240
    # tracks at different rates: a lagging noise track bounds the source
    assert E(4801, 3, 1000, 21, 21) == 240 * ((1000 - 255) // 240)
    # one-sample pushes on top change nothing until a frame closes
    assert E(4802, 3, None, 21, 21) == E(4801, 3, None, 21, 21)
    # no noise filter: noise = the oscillator bound
    assert emit_count(geometry(fir_taps=0), 4801, 2, None, 0, 21, 21) == 2160


def test_latency_formula_is_a_bound_and_tight():
    from golf_amd.stream import emit_count, stream_latency

    for kw in ({}, dict(fir_taps=0), dict(phase_hop=240, w_hop=480), dict(os=1, half=0, w_hop=240, fir_hop=120)):
        g = geometry(**kw)
        L = stream_latency(g)

        def E(S):  # every track pushed up to input time S
            return emit_count(g, S // g.phase_hop + 1, S // g.w_hop + 1, S + 1, S // g.fir_hop + 1, S // g.hop + 1,
                              S // g.hop + 1)

        worst = 0
        for t in range(0, 3 * max(g.w_hop, g.hop, g.phase_hop) * 4):
            assert E(t + L) > t, (kw, t)
            need = next(s for s in range(t, t + L + 1) if E(s) > t)
            worst = max(worst, need - t)
        assert worst <= L, (kw, worst, L)
        if not kw:   # golf-ss: within one LPC frame of the worst case actually met
            assert L - g.hop < worst, (worst, L)
    assert stream_latency(geometry()) == 2655


def test_final_lengths_match_the_one_shot_helpers():
    from golf_amd import functional as GF
    from golf_amd.stream import final_lengths

    g = geometry()
    fl = final_lengths(g, 48000, None, 200, 200)
    assert fl["osc"] == GF.osc_lengths(48000, 1, 4)[1] == 48000
    assert fl["noise_filter"] == GF.fir_frames_length(48000, 200, 510, 240) == 47760
    assert fl["out"] == GF.ss_output_length(47760, 200, 240) == 47760
    fl = final_lengths(geometry(fir_taps=0), 48000, 47000, 0, 200)
    assert fl["noise"] == 47000 and fl["out"] == 47000
    fl = final_lengths(geometry(fir_taps=0), 48000, None, 0, 200)
    assert fl["out"] == 199 * 240 + 1
    for T, F in ((12345, 60), (4800, 20), (1000, 3)):
        assert final_lengths(g, T, None, F, F)["noise_filter"] == GF.fir_frames_length(T, F, 510, 240)


def test_refusals():
    import torch

    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import (LTVAPZeroPhaseFIRFilter, LTVMinimumPhaseFIRFilter, LTVMinimumPhaseFIRFilterPrecise,
                                  LTVZeroPhaseFIRFilter, LTVZeroPhaseFIRFilterPrecise)
    from golf_amd.noise import UniformNoise
    from golf_amd.sf import HarmonicPlusNoiseSynth
    from golf_amd.stream import DecoderStream, _branch_kind
    from golf_amd.synth import WrappedPhaseDownsampledIndexedGlottalFlowTable
    from golf_amd.synthetic import make_ddsp_decoder, make_decoder

    with pytest.raises(NotImplementedError, match="LTVMinimumPhaseFilter"):
        DecoderStream(make_decoder(framewise=True), 2)
    d = make_ddsp_decoder()
    with pytest.raises(NotImplementedError, match="HarmonicPlusNoiseSynth"):
        DecoderStream(d, 2)
    assert isinstance(d, HarmonicPlusNoiseSynth)
    d = make_decoder()
    d.subtract_harmonics = True
    with pytest.raises(NotImplementedError, match="subtract_harmonics"):
        DecoderStream(d, 2)
    d = make_decoder()
    d.harm_oscillator = WrappedPhaseDownsampledIndexedGlottalFlowTable(hop_rate=10, in_channels=4, points=64, table_size=4)
    with pytest.raises(NotImplementedError, match="WrappedPhase"):
        DecoderStream(d, 2)
    d = make_decoder()
    d.noise_generator = UniformNoise()
    with pytest.raises(NotImplementedError, match="UniformNoise"):
        DecoderStream(d, 2)
    d = make_decoder()
    d.noise_filter = LTVZeroPhaseFIRFilterPrecise(window="hanning", n_mag=256)
    with pytest.raises(NotImplementedError, match="LTVZeroPhaseFIRFilterPrecise"):
        DecoderStream(d, 2)
    # a filter streams as the frame-wise zero-phase FIR only if it runs that class's own forward
    for cls in (LTVZeroPhaseFIRFilter, LTVAPZeroPhaseFIRFilter):
        assert _branch_kind(cls(window="hanning", n_mag=256)) == "fir"
    for cls in (LTVZeroPhaseFIRFilterPrecise, LTVMinimumPhaseFIRFilter, LTVMinimumPhaseFIRFilterPrecise):
        assert _branch_kind(cls(window="hanning", n_mag=256)) is None
    st = DecoderStream(make_decoder(), 2)
    z = lambda *s: AudioTensor(torch.zeros(*s))
    args = dict(phase=z(2, 1), harm_oscillator_params=(AudioTensor(torch.zeros(2, 1), 2400),),
                noise_filter_params=(AudioTensor(torch.zeros(2, 1, 256), 240),),
                end_filter_params=(AudioTensor(torch.zeros(2, 1), 240), AudioTensor(torch.zeros(2, 1, 22), 240)))
    with pytest.raises(NotImplementedError, match="voicing"):
        st.push(**args, voicing=z(2, 1))
    g = AudioTensor(torch.zeros(2, 1, requires_grad=True), 240)
    with pytest.raises(NotImplementedError, match="requires grad"):
        st.push(**{**args, "end_filter_params": (g, args["end_filter_params"][1])})
    with pytest.raises(Exception, match="ROCm device"):   # CPU tensors: there is no CPU path
        st.push(**args)


def test_state_entries_refuse_bad_arguments_without_launch():
    import ctypes

    from golf_amd import _lib

    lib = _lib.load()
    f = lib.golf_ltv_allpole_fwd_state_f32
    one = ctypes.c_void_p(256)   # never dereferenced: every call below is refused on its arguments
    assert f(one, 10, one, one, one, 10, 2, 10, 3, 4, 8, None, None) == -1 and b"null" in lib.golf_last_error()
    assert f(one, 10, one, one, one, 10, 2, 10, 3, 99, 8, one, None) == -3
    assert f(one, 10, one, one, one, 10, 2, 0, 3, 4, 8, one, None) == -1
    assert f(one, 100, one, one, one, 100, 2, 100, 3, 4, 10, one, None) == -1 and b"exceeds" in lib.golf_last_error()
    assert f(one, 5, one, one, one, 10, 2, 10, 3, 4, 8, one, None) == -1 and b"stride" in lib.golf_last_error()
    o = lib.golf_glottal_osc_stream_f32
    ok = [one, 11, 10, 0, 1, 4, one, 3, 3, 0, 2400, one, 100, 2048, 1, 0, one, one, 40, None, 2, None]
    call = lambda kw: o(*[kw.get(i, v) for i, v in enumerate(ok)])
    assert call({16: None}) == -1 and b"null" in lib.golf_last_error()           # acc
    assert call({2: 0, 3: 0}) == -1                                               # nothing to render
    assert call({3: 2}) == -1
    assert call({1: 5}) == -1 and b"stride" in lib.golf_last_error()
    assert call({18: 39}) == -1 and b"stride" in lib.golf_last_error()
    assert call({9: 1}) == -1 and b"row" in lib.golf_last_error()                # rows start after the first needed one
    assert call({12: 1}) == -1
