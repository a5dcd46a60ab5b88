"""GPU: the block-by-block harmonic-plus-noise analysis -- golf_harmonic_analysis_stream_f32 on windows of the inputs against
the one-shot entry's rows, analysis_stream.HarmonicNoiseStream against hna.HarmonicNoiseAnalysis under random cuts of both
inputs, and the live chain F0TrackerStream -> HarmonicNoiseStream -> HarmonicPlusNoiseStream on the DDSP decoder.

Every comparison of the analysis is ``torch.equal``: a frame's arithmetic does not depend on where the buffers start.  The
one-shot entry's own results are held by tests/test_gpu_hna.py, which this change leaves as it was."""
import numpy as np
import pytest
import torch

import hna_ref as R

pytestmark = pytest.mark.gpu

SR = 16000.0


def small_inputs():
    """B = 3, T = 700, hop 16, F = 44: a glide with unvoiced gaps (two-sided chirps, one-sided ones at both ends of every voiced
    run, at the first and at the last frame too), an all-unvoiced row, and a low-f0 row whose window saturates at max_window =
    128 (4 periods of 300 Hz are 213 samples)."""
    T, hop = 700, 16
    F = T // hop + 1
    glide = 600.0 * (1000.0 / 600.0) ** (np.arange(F) / (F - 1.0))    # curved: the one- and two-sided chirps differ
    low = np.full(F, 300.0)
    x = np.array([R.voice(glide, T, 6, 11, 0.05, hop, SR), 0.2 * np.random.default_rng(5).normal(0, 1, T),
                  R.voice(low, T, 8, 12, 0.05, hop, SR)]).astype(np.float32)
    f0 = np.array([glide, np.zeros(F), low], np.float32)
    f0[0, [4, 5, 9, 20, 21, 22, 30, 32]] = 0    # runs of one frame (no voiced neighbour) and longer ones
    return x, f0


SMALL = dict(sample_rate=SR, hop=16, K=5, n_mag=9, max_window=128, unvoiced_window=64)
_cases = {}


def case(name):
    """name -> (x (B, T) and f0 (B, F) on the device, keyword arguments of the functional entries)."""
    if name in _cases:
        return _cases[name]
    if name in ("small", "K256", "n_mag513", "smooth"):
        x, f0 = small_inputs()
        kw = dict(SMALL, **{"K256": dict(K=256), "n_mag513": dict(n_mag=513), "smooth": dict(smooth=3)}.get(name, {}))
    elif name == "L1600":     # 4 periods of 60 Hz at 24 kHz: staging strides over the workgroup; a second row clamps at 2048
        F = 21
        tr = [np.full(F, 60.0), np.full(F, 40.0)]
        x = np.array([R.voice(t, 4800, 10, 200 + i) for i, t in enumerate(tr)]).astype(np.float32)
        f0 = np.array(tr, np.float32)
        f0[0, 12] = 0
        kw = dict(sample_rate=R.SR, hop=R.HOP, K=12, n_mag=33, max_window=2048, unvoiced_window=960)
    elif name == "recipe":    # hop 240, K = 155, n_mag = 256, B = 2, one second
        F = 101
        tr = [np.linspace(90.0, 140.0, F), 220.0 * 2 ** (0.04 * np.sin(0.3 * np.arange(F)))]
        x = np.array([R.voice(t, 24000, 40, 300 + i) for i, t in enumerate(tr)]).astype(np.float32)
        f0 = np.array(tr, np.float32)
        f0[0, 30:37] = 0
        f0[1, [0, 1, 50, 99, 100]] = 0
        kw = dict(sample_rate=R.SR, hop=R.HOP, K=155, n_mag=256, max_window=2048, unvoiced_window=960)
    _cases[name] = (torch.tensor(x).cuda(), torch.tensor(f0).cuda(), kw)
    return _cases[name]


def args(kw):
    kw = dict(kw)
    return (kw.pop("sample_rate"), kw.pop("hop"), kw.pop("K")), kw


def one_shot(x, f0, kw):
    from golf_amd import functional as GF

    pos, kw = args(kw)
    return GF.harmonic_analysis(x, f0, *pos, return_phases=True, **kw)


def window(x, f0, kw, f_first, n, x_t0, x_end, f0_first, f0_end, last, strided=False, phases=True):
    """The stream entry on samples [x_t0, x_end) and f0 frames [f0_first, f0_end) of (x, f0)."""
    from golf_amd import functional as GF

    def view(t, lo, hi, extra):
        if not strided:
            return t[:, lo:hi]
        buf = torch.full((t.shape[0], hi - lo + extra), float("nan"), device="cuda")
        buf[:, : hi - lo] = t[:, lo:hi]
        return buf[:, : hi - lo]

    pos, kw = args(kw)
    return GF.harmonic_analysis_stream(view(x, x_t0, x_end, 37), view(f0, f0_first, f0_end, 5), x_t0, f_first, f0_first, n, last,
                                       *pos, return_phases=phases, **kw)


def random_windows(T, F, hop, Lmax, rng):
    """Consecutive windows of frames with admissible positions drawn at random: (f_first, n, x_t0, x_end, f0_first, f0_end,
    last).  A window that is not the last ends where its frames' longest window and next neighbour still lie in (x, f0)."""
    out, f = [], 0
    while f < F:
        n = int(rng.integers(1, 7))
        f_end = min(f + n, F)
        need = (f_end - 1) * hop + Lmax - Lmax // 2
        x_t0 = int(rng.integers(0, max(f * hop - Lmax // 2, 0) + 1))
        f0_first = int(rng.integers(0, max(f - 1, 0) + 1))
        if need <= T and f_end + 1 <= F:
            out.append((f, f_end - f, x_t0, int(rng.integers(need, T + 1)), f0_first, int(rng.integers(f_end + 1, F + 1)), False))
            f = f_end
        else:
            out.append((f, F - f, x_t0, T, f0_first, F, True))
            f = F
    return out


def check_windows(name, seed, strided=False):
    x, f0, kw = case(name)
    ref = one_shot(x, f0, kw)
    Lmax = max(kw["max_window"], kw["unvoiced_window"])
    wins = random_windows(x.shape[1], f0.shape[1], kw["hop"], Lmax, np.random.default_rng(seed))
    assert len(wins) >= 3 and not wins[0][-1] and wins[-1][-1]
    assert any(w[2] > 0 for w in wins) and any(w[4] > 0 for w in wins)
    for f_first, n, *where, last in wins:
        got = window(x, f0, kw, f_first, n, *where, last, strided=strided)
        assert len(got) == len(ref) == 3
        for g, r in zip(got, ref):
            assert torch.equal(g, r[:, f_first:f_first + n]), (name, f_first, n, where, last)
    return ref


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_entry_windows_equal_the_one_shot_rows(seed):
    x, f0, kw = case("small")
    ref = check_windows("small", seed)
    # the rows are what the docstring says
    rules = R.analyse(x.cpu().numpy(), f0.cpu().numpy(), **kw)
    assert {"central", "forward", "backward", "none", "unvoiced"} <= set(rules["rule"][0])
    assert rules["rule"][0][0] == "forward" and rules["rule"][0][-1] == "backward"
    assert (rules["L"][1] == 64).all() and not rules["voiced"][1].any() and (rules["L"][2] == 128).all()
    assert (ref[0][1] == 0).all() and (ref[0][0] > 0).any() and (ref[0][2] > 0).any()


@pytest.mark.parametrize("name", ["L1600", "K256", "n_mag513", "smooth"])
def test_entry_at_the_tile_edges(name):
    x, f0, kw = case(name)
    check_windows(name, 3)
    if name == "L1600":
        L = R.analyse(x.cpu().numpy(), f0.cpu().numpy(), **kw)["L"]
        assert L[0].max() == 1600 and L[0].min() == 960 and (L[1] == 2048).all()


def test_entry_strided_rows():
    check_windows("small", 4, strided=True)


def test_entry_boundary_frames():
    x, f0, kw = case("small")
    (T, F), hop, Lmax = (x.shape[1], f0.shape[1]), kw["hop"], 128
    ref = one_shot(x, f0, kw)
    # frame 0 alone, from the smallest buffers that hold it: zeros stand before sample 0, there is no previous neighbour
    got = window(x, f0, kw, 0, 1, 0, Lmax - Lmax // 2, 0, 2, False)
    assert all(torch.equal(g, r[:, :1]) for g, r in zip(got, ref))
    # the last frame of a shorter utterance (x[:, :Ts], f0[:, :Fs]): no next neighbour, zeros after Ts ...
    Fs, Ts = F - 4, (F - 5) * hop + 9
    assert f0[0, Fs - 2] > 0 and f0[0, Fs - 1] > 0 and f0[0, Fs] > 0 and f0[2, Fs] > 0
    short = one_shot(x[:, :Ts], f0[:, :Fs], kw)
    lo = (Fs - 1) * hop - Lmax // 2
    as_last = window(x, f0, kw, Fs - 1, 1, lo, Ts, Fs - 2, Fs, True)
    assert all(torch.equal(g, r[:, Fs - 1:]) for g, r in zip(as_last, short))
    # ... and the same frame as a frame in the middle of the longer one: a two-sided chirp and real samples after Ts
    inner = window(x, f0, kw, Fs - 1, 1, lo, (Fs - 1) * hop + Lmax // 2, Fs - 2, Fs + 1, False)
    assert all(torch.equal(g, r[:, Fs - 1:Fs]) for g, r in zip(inner, ref))
    for row in (0, 2):     # voiced rows: the chirp (row 0) and the padding (both) differ
        assert not torch.equal(inner[0][row], as_last[0][row]) and not torch.equal(inner[2][row], as_last[2][row])
    assert not torch.equal(inner[2][1], as_last[2][1]) and torch.equal(inner[0][1], as_last[0][1])   # unvoiced: padding only
    # the next neighbour alone, on the same samples
    chirp_only = window(x, f0, kw, Fs - 1, 1, lo, (Fs - 1) * hop + Lmax // 2, Fs - 2, Fs, True)
    assert not torch.equal(chirp_only[0][0], inner[0][0]) and torch.equal(chirp_only[0][1], inner[0][1])
    assert torch.equal(chirp_only[0][2], inner[0][2])      # a constant f0: the chirp is 0 either way


def test_entry_null_outputs_untouched():
    from golf_amd import _lib

    lib = _lib.load()
    x, f0, kw = case("small")
    B, K, n_mag, hop = x.shape[0], kw["K"], kw["n_mag"], kw["hop"]
    ref = one_shot(x, f0, kw)
    f_first, n, x_t0, f0_first = 10, 6, 90, 8
    xs, fs = x[:, x_t0:340], f0[:, f0_first:20]

    def call(amp, phases, log_mag):
        rc = lib.golf_harmonic_analysis_stream_f32(xs.data_ptr(), xs.stride(0), x_t0, xs.shape[1], fs.data_ptr(), fs.stride(0),
                                                   f0_first, fs.shape[1], amp.data_ptr(), _lib.ptr(phases), _lib.ptr(log_mag),
                                                   B, f_first, n, 0, K, n_mag, hop, 4, 2 * hop, 128, 64, 0, SR, 1e-12,
                                                   _lib.stream_ptr())
        _lib.check(rc, "golf_harmonic_analysis_stream_f32")

    def fresh():
        return [torch.full((B, n, m), float("nan"), device="cuda") for m in (K, K, n_mag, 7)]

    full = fresh()
    call(*full[:3])
    assert all(torch.equal(t, r[:, f_first:f_first + n]) for t, r in zip(full[:3], ref)) and torch.isnan(full[3]).all()
    for keep in ((1,), (2,), ()):
        part = fresh()
        call(part[0], *(part[i] if i in keep else None for i in (1, 2)))
        assert torch.equal(part[0], full[0])
        for i in (1, 2):
            assert torch.equal(part[i], full[i]) if i in keep else torch.isnan(part[i]).all()


def test_entry_refuses_without_a_launch():
    from golf_amd import _lib
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError

    lib = _lib.load()
    x, f0, kw = case("small")
    B, K, n_mag, hop, Lmax = x.shape[0], kw["K"], kw["n_mag"], kw["hop"], 128
    f_first, n = 10, 6
    lo, need = f_first * hop - Lmax // 2, (f_first + n - 1) * hop + Lmax - Lmax // 2      # 96 and 304
    good = dict(x_t0=lo, x_end=need, f0_first=f_first - 1, f0_end=f_first + n + 1, last=False)
    amp, ph, lm = (torch.full((B, n, m), float("nan"), device="cuda") for m in (K, K, n_mag))

    def c_call(x_t0, x_end, f0_first, f0_end, last, f_first=f_first):
        xs, fs = x[:, max(x_t0, 0):x_end], f0[:, max(f0_first, 0):f0_end]
        return lib.golf_harmonic_analysis_stream_f32(xs.data_ptr(), xs.stride(0), x_t0, xs.shape[1], fs.data_ptr(),
                                                     fs.stride(0), f0_first, fs.shape[1], amp.data_ptr(), ph.data_ptr(),
                                                     lm.data_ptr(), B, f_first, n, int(last), K, n_mag, hop, 4, 2 * hop, 128,
                                                     64, 0, SR, 1e-12, _lib.stream_ptr())

    for bad, word in ((dict(x_t0=lo + 1), "x_t0"),                                # a frame could read below the buffer
                      (dict(f0_first=f_first), "f0_first"),                       # the previous neighbour is missing
                      (dict(f0_end=f_first + n - 1, last=True), "n_f0"),          # f0 does not cover the frames
                      (dict(x_end=need - 1), "n_x"),                              # a window could reach beyond the buffer
                      (dict(f0_end=f_first + n), "n_f0"),                         # the next neighbour has not come
                      (dict(x_t0=-1), "x_t0"), (dict(f0_first=-1), "f0_first")):
        a = dict(good, **bad)
        assert c_call(**a) == -1, bad                                             # GOLF_EINVAL
        assert word.encode() in lib.golf_last_error(), (bad, lib.golf_last_error())
        with pytest.raises(GolfError, match=word):
            GF.harmonic_analysis_stream(x[:, max(a["x_t0"], 0):a["x_end"]], f0[:, max(a["f0_first"], 0):a["f0_end"]],
                                        a["x_t0"], f_first, a["f0_first"], n, a["last"], SR, hop, K, n_mag=n_mag,
                                        max_window=128, unvoiced_window=64)
    assert c_call(**dict(good, x_t0=0, f0_first=1), f_first=0) == -1 and b"f0_first" in lib.golf_last_error()
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in (amp, ph, lm))                       # nothing was launched
    # each of them is accepted at its limit, with and without last
    assert c_call(**good) == 0
    assert c_call(**dict(good, x_end=need - 50, f0_end=f_first + n, last=True)) == 0
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in (amp, ph, lm))


# ---- the stream ------------------------------------------------------------------------------------------------------------
def module(kw, n_mag=True):
    from golf_amd.hna import HarmonicNoiseAnalysis

    return HarmonicNoiseAnalysis(kw["sample_rate"], kw["hop"], kw["K"], n_mag=kw["n_mag"] if n_mag else None,
                                 max_window=kw["max_window"], unvoiced_window=kw["unvoiced_window"],
                                 smooth=kw.get("smooth", 0)).cuda()


def cuts(n, sizes, rng):
    out = []
    while sum(out) < n:
        out.append(min(int(rng.choice(sizes)), n - sum(out)))
    return out


def stream_run(st, x, f0, mode, seed, plain=True):
    """Push (x, f0) through ``st`` in seeded random cuts of each, finish, and concatenate: ``mixed`` interleaves the two at
    random, ``late`` delivers a frame's f0 eight frames after its last sample, ``f0 first`` / ``audio first`` deliver one input
    whole before the other starts."""
    rng = np.random.default_rng(seed)
    hop, Lmax = st.hop, st.span
    (T, F) = x.shape[1], f0.shape[1]
    xs = cuts(T, [0, 1, 1, hop, Lmax // 2, Lmax + 3, 3 * Lmax + 1], rng)
    fs = cuts(F, [0, 1, 2, 3, 10], rng)
    push = st.push_all if plain else st.push
    outs, px, pf = [], 0, 0
    if mode == "late":
        for n in xs:
            k = max(min((px + n) // hop - 8, F) - pf, 0)
            outs.append(push(x[:, px:px + n], f0[:, pf:pf + k]))
            px, pf = px + n, pf + k
        outs.append(push(f0=f0[:, pf:]))
        pf = F
    else:
        ev = [("x", n) for n in xs] + [("f", n) for n in fs]
        if mode == "mixed":
            ev = [ev[i] for i in rng.permutation(len(ev))]
        elif mode == "f0 first":
            ev = [("f", F)] + ev[:len(xs)]
        elif mode == "audio first":
            ev = [("x", T)] + ev[len(xs):]
        for kind, n in ev:
            if kind == "x":
                outs.append(push(x=x[:, px:px + n]))
                px += n
            else:
                outs.append(push(f0=f0[:, pf:pf + n]))
                pf += n
    assert px == T and pf == F
    outs.append(st.finish_all() if plain else st.finish())
    if not plain:
        from golf_amd.audiotensor import AudioTensor

        outs = [o if isinstance(o, tuple) else (o,) for o in outs]
        assert all(isinstance(t, AudioTensor) and t.hop_length == hop for o in outs for t in o)
        outs = [tuple(t.as_tensor() for t in o) for o in outs]
    assert any(o[0].shape[1] == 0 for o in outs) and sum(o[0].shape[1] > 0 for o in outs) >= 2
    return tuple(torch.cat([o[i] for o in outs], 1) for i in range(len(outs[0])))


@pytest.mark.parametrize("name", ["small", "L1600", "K256", "n_mag513", "smooth", "recipe"])
def test_stream_equals_the_module(name):
    from golf_amd.analysis_stream import HarmonicNoiseStream, open_analysis_stream

    x, f0, kw = case(name)
    m = module(kw)
    three = m.analyse(x, f0)
    fwd = tuple(t.as_tensor() for t in m(x, f0))
    assert torch.equal(fwd[0], three[0]) and torch.equal(fwd[1], three[2])
    st = open_analysis_stream(m, x.shape[0])
    assert type(st) is HarmonicNoiseStream
    # one stream, one utterance after the other: every delivery, two cut sequences of the same one
    for mode, seed in (("mixed", 1), ("mixed", 2), ("late", 3), ("f0 first", 4), ("audio first", 5)):
        got = stream_run(st, x, f0, mode, seed)
        assert len(got) == 3 and all(torch.equal(g, w) for g, w in zip(got, three)), (name, mode)
    got = stream_run(st, x, f0, "mixed", 6, plain=False)      # push / finish: the types of forward
    assert len(got) == 2 and all(torch.equal(g, w) for g, w in zip(got, fwd))
    # a row alone
    for b in range(x.shape[0]):
        alone = stream_run(HarmonicNoiseStream(m, 1), x[b:b + 1], f0[b:b + 1], "mixed", 7)
        assert all(torch.equal(a[0], w[b]) for a, w in zip(alone, three))


def test_stream_amplitudes_alone_lengths_and_refusals():
    from golf_amd._lib import GolfError
    from golf_amd.analysis_stream import HarmonicNoiseStream
    from golf_amd.audiotensor import AudioTensor

    x, f0, kw = case("small")
    m = module(kw, n_mag=False)
    st = HarmonicNoiseStream(m, 3)
    want = m(x, f0).as_tensor()
    got = stream_run(st, x, f0, "mixed", 8, plain=False)
    assert len(got) == 1 and torch.equal(got[0], want)
    # the utterance is the f0 frames received: more frames than samples, more samples than frames, no frame, nothing at all
    for T, F in ((100, 44), (700, 12), (700, 0), (0, 0), (0, 3)):
        a = st.push(AudioTensor(x[:, :T]), AudioTensor(f0[:, :F], 16))
        b = st.finish()
        out = torch.cat([a.as_tensor(), b.as_tensor()], 1)
        assert out.shape == (3, F, 5) and out.is_cuda
        if F:
            assert torch.equal(out, m(x[:, :T], f0[:, :F]).as_tensor())
    out = st.finish_all()                                      # a stream that was given nothing
    assert [tuple(t.shape) for t in out] == [(3, 0, 5), (3, 0, 5)]
    # autocast: half precision is cast as the one-shot functions cast it; outside it is refused
    with torch.autocast("cuda", dtype=torch.bfloat16):
        a = st.push(x.bfloat16(), f0.bfloat16())
        b = st.finish()
    assert torch.equal(torch.cat([a.as_tensor(), b.as_tensor()], 1), m(x.bfloat16().float(), f0.bfloat16().float()).as_tensor())
    with pytest.raises(GolfError, match="fp32"):
        st.push(x=x.bfloat16())
    with pytest.raises(GolfError, match="fp32"):
        st.push(f0=f0.double())
    with pytest.raises(NotImplementedError, match="requires grad"):
        st.push(x=x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="B=3"):
        st.push(x=x[:2])
    with pytest.raises(AssertionError, match="hop 16"):
        st.push(f0=AudioTensor(f0, 8))
    assert (st.pushed, st.f0_received, st.framed) == (0, 0, 0)


# ---- end to end --------------------------------------------------------------------------------------------------------------
def test_live_resynthesis_chain_on_the_ddsp_decoder():
    """F0TrackerStream(lag=8) -> HarmonicNoiseStream -> HarmonicPlusNoiseStream, block by block, against the one-shot chain on
    the same fixed-lag f0 (F0TrackerStream given the whole waveform -> HarmonicNoiseAnalysis -> the decoder's ``forward``): the
    controls and the audio are ``torch.equal``, and so is the audio of the decoder's stream given everything in one push."""
    from golf_amd.analysis_stream import F0TrackerStream, HarmonicNoiseStream
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.f0 import F0Tracker
    from golf_amd.hna import HarmonicNoiseAnalysis
    from golf_amd.stream import HarmonicPlusNoiseStream
    from golf_amd.synthetic import make_ddsp_decoder

    B, T, hop, sr, K = 2, 12000, R.HOP, R.SR, 155
    F = T // hop + 1
    tr = [np.linspace(110.0, 160.0, F), 200.0 * 2 ** (0.03 * np.sin(0.4 * np.arange(F)))]
    x = torch.tensor(np.array([R.voice(t, T, 30, 700 + i) for i, t in enumerate(tr)]).astype(np.float32)).cuda()
    x[0, 5000:7000] = 0      # a silent stretch
    noise = torch.randn(B, T + 4 * hop, generator=torch.Generator().manual_seed(4)).cuda()
    dec = make_ddsp_decoder(K, injected_noise=noise).cuda().eval()
    with torch.no_grad():
        dec.end_filter.kernel.copy_(0.1 * torch.randn(dec.end_filter.kernel.shape, generator=torch.Generator().manual_seed(5))
                                    * torch.exp(-0.05 * torch.arange(dec.end_filter.kernel.shape[-1])))
    tracker = F0Tracker(sr, hop).cuda()
    hna = HarmonicNoiseAnalysis(sr, hop, K, n_mag=256).cuda()

    def decode(st, f0, amp, log_mag, nz):
        return st.push(phase=AudioTensor(f0 / sr, hop), harm_oscillator_params=(AudioTensor(amp, hop),),
                       noise_filter_params=(AudioTensor(log_mag, hop),), noise=AudioTensor(nz))

    # the one-shot chain on the fixed-lag f0
    f0_st = F0TrackerStream(tracker, B, lag=8)
    f0_all = torch.cat([f0_st.push(x).as_tensor(), f0_st.finish().as_tensor()], 1)
    assert f0_all.shape == (B, F) and (f0_all > 0).any()
    amp_all, lm_all = (t.as_tensor() for t in hna(x, f0_all))
    whole = HarmonicPlusNoiseStream(dec, B)
    y_ref = torch.cat([decode(whole, f0_all, amp_all, lm_all, noise), whole.finish()], 1)

    # the live chain
    hna_st, out = HarmonicNoiseStream(hna, B), HarmonicPlusNoiseStream(dec, B)
    f0s, amps, lms, ys, pos = [], [], [], [], 0
    for n in (2400, 1, 0, 2399, 3000, 600, 3600):
        block, nz = x[:, pos:pos + n], noise[:, pos:pos + n]
        pos += n
        f0 = f0_st.push(block)
        amp, lm = hna_st.push(block, f0)
        ys.append(decode(out, f0.as_tensor(), amp.as_tensor(), lm.as_tensor(), nz))
        f0s.append(f0.as_tensor()), amps.append(amp.as_tensor()), lms.append(lm.as_tensor())
    assert pos == T
    f0 = f0_st.finish()
    amp, lm = hna_st.push(f0=f0)
    amp2, lm2 = hna_st.finish()
    f0s.append(f0.as_tensor())
    amps += [amp.as_tensor(), amp2.as_tensor()]
    lms += [lm.as_tensor(), lm2.as_tensor()]
    ys.append(decode(out, f0.as_tensor(), torch.cat(amps[-2:], 1), torch.cat(lms[-2:], 1), noise[:, pos:]))
    ys.append(out.finish())
    assert torch.equal(torch.cat(f0s, 1), f0_all)
    assert torch.equal(torch.cat(amps, 1), amp_all) and torch.equal(torch.cat(lms, 1), lm_all)
    assert sum(a.shape[1] > 0 for a in amps[:-2]) >= 3       # frames came out while the audio was still coming in
    y = torch.cat(ys, 1)
    assert y.shape == y_ref.shape and y.shape[1] > T - 2 * hop and torch.isfinite(y).all() and float(y.abs().max()) > 1e-3
    assert torch.equal(y, y_ref)
    with torch.no_grad():
        one = dec(phase=AudioTensor(f0_all / sr, hop), harm_oscillator_params=(AudioTensor(amp_all, hop),),
                  noise_generator_params=(), harm_filter_params=(), noise_filter_params=(AudioTensor(lm_all, hop),)).as_tensor()
    assert torch.equal(y, one)
