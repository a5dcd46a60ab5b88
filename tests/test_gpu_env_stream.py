"""GPU: the spectral-envelope analysis at a position of a longer utterance (golf_spectral_envelope_stream_f32,
functional.spectral_envelope_stream) and block by block (analysis_stream.SpectralEnvelopeStream): every frame has the bits
of the one-shot call (tests/test_gpu_env.py pins those against the float64 restatement), whatever the window or the cuts;
and the NHV live loop, F0TrackerStream -> SpectralEnvelopeStream + HarmonicNoiseStream -> HarmonicPlusNoiseStream."""
import numpy as np
import pytest
import torch

import env_ref as R

pytestmark = pytest.mark.gpu


def dev(a):
    return a if isinstance(a, torch.Tensor) else torch.tensor(a).cuda()


def one_shot(name):
    from golf_amd import functional as GF

    x, f0, kw = R.cases()[name]
    kw = dict(dict(n_ceps=kw["n_fft"] // 2 + 1), **kw)
    return dev(x), dev(f0), kw, GF.spectral_envelope(dev(x), dev(f0), **kw)


def hwmax_of(kw):
    from golf_amd import functional as GF

    return GF.spectral_envelope_hwmax(kw["sample_rate"], kw["n_fft"], kw.get("f0_floor"))


def random_windows(T, F, hop, hwmax, rng, n=4):
    """(f_first, n_frames, x_t0, x_end, f0_first, f0_end, last): windows without ``last`` where the samples allow one, then
    windows that end the utterance."""
    out = []
    n_open = (T - hwmax - 1) // hop + 1 if T >= hwmax + 1 else 0   # frames whose longest window ends inside the signal
    for _ in range(n):
        if min(n_open, F) < 1:
            break
        f_first = int(rng.integers(0, min(n_open, F)))
        k = int(rng.integers(1, min(n_open, F) - f_first + 1))
        x_t0 = int(rng.integers(0, max(f_first * hop - hwmax, 0) + 1))
        x_end = int(rng.integers((f_first + k - 1) * hop + hwmax + 1, T + 1))
        out.append((f_first, k, x_t0, x_end, int(rng.integers(0, f_first + 1)), int(rng.integers(f_first + k, F + 1)), False))
    for _ in range(2):
        f_first = int(rng.integers(0, F))
        k = int(rng.integers(1, F - f_first + 1))
        x_t0 = min(max(f_first * hop - hwmax, 0), T)
        out.append((f_first, k, x_t0, T, f_first, int(rng.integers(f_first + k, F + 1)), True))
    return out


@pytest.mark.parametrize("name", list(R.cases()))
def test_entry_windows_equal_the_one_shot_rows(name):
    from golf_amd import functional as GF

    x, f0, kw, (env, ceps) = one_shot(name)
    (T, F), hop = (x.shape[1], f0.shape[1]), kw["hop"]
    more = {k: v for k, v in kw.items() if k not in ("sample_rate", "hop")}
    wins = random_windows(T, F, hop, hwmax_of(kw), np.random.default_rng(len(name)))
    assert len(wins) >= 3 or T < 2 * hwmax_of(kw)
    for f_first, k, x_t0, x_end, f0_first, f0_end, last in wins:
        got = GF.spectral_envelope_stream(x[:, x_t0:x_end], f0[:, f0_first:f0_end], x_t0, f_first, f0_first, k, last,
                                          kw["sample_rate"], hop, **more)
        sl = slice(f_first, f_first + k)
        assert torch.equal(got[0], env[:, sl]) and torch.equal(got[1], ceps[:, sl]), (name, f_first, k, x_t0, last)


def test_entry_strided_rows_each_output_alone_and_null_outputs_untouched():
    from golf_amd import _lib
    from golf_amd import functional as GF

    x, f0, kw, (env, ceps) = one_shot("n256")
    (B, T), F, hop, n, hw = x.shape, f0.shape[1], kw["hop"], kw["n_fft"], hwmax_of(kw)
    more = {k: v for k, v in kw.items() if k not in ("sample_rate", "hop")}
    f_first, k = 3, 3
    x_t0, x_end = f_first * hop - hw, (f_first + k - 1) * hop + hw + 1
    assert x_t0 > 0 and x_end <= T
    wide_x = torch.full((B, x_end - x_t0 + 37), float("nan"), device="cuda")
    wide_x[:, :x_end - x_t0] = x[:, x_t0:x_end]
    wide_f = torch.full((B, k + 5), float("nan"), device="cuda")
    wide_f[:, :k] = f0[:, f_first:f_first + k]
    xv, fv = wide_x[:, :x_end - x_t0], wide_f[:, :k]
    assert not xv.is_contiguous() and not fv.is_contiguous()
    args = (xv, fv, x_t0, f_first, f_first, k, False, kw["sample_rate"], hop)
    got = GF.spectral_envelope_stream(*args, **more)
    sl = slice(f_first, f_first + k)
    assert torch.equal(got[0], env[:, sl]) and torch.equal(got[1], ceps[:, sl])
    assert torch.equal(GF.spectral_envelope_stream(*args, **dict(more, n_ceps=None)), env[:, sl])
    assert torch.equal(GF.spectral_envelope_stream(*args, **dict(more, n_ceps=7), return_log_env=False), ceps[:, sl, :7])
    # through the ABI: a NULL output is not written, and nothing beyond the other
    lib = _lib.load()
    lo, hi = R.defaults(kw["sample_rate"], n)
    xc, fc = xv.contiguous(), fv.contiguous()

    def call(e, c, n_ceps):
        rc = lib.golf_spectral_envelope_stream_f32(xc.data_ptr(), xc.stride(0), x_t0, xc.shape[1], fc.data_ptr(), fc.stride(0),
                                                   f_first, k, _lib.ptr(e), _lib.ptr(c), B, f_first, k, 0, n, n_ceps, hop,
                                                   kw["sample_rate"], lo, hi, kw["unvoiced_f0"], -0.15, 1e-12, R.OFFSET,
                                                   _lib.stream_ptr())
        _lib.check(rc, "golf_spectral_envelope_stream_f32")

    pad = 16
    e_buf = torch.full((B * k * (n // 2 + 1) + 2 * pad,), float("nan"), device="cuda")
    c_buf = torch.full((B * k * 7 + 2 * pad,), float("nan"), device="cuda")
    call(e_buf[pad:], None, 0)
    assert torch.equal(e_buf[pad:-pad].view(B, k, -1), env[:, sl]) and torch.isnan(e_buf[:pad]).all() and torch.isnan(e_buf[-pad:]).all()
    call(None, c_buf[pad:], 7)
    assert torch.equal(c_buf[pad:-pad].view(B, k, 7), ceps[:, sl, :7]) and torch.isnan(c_buf[:pad]).all() and torch.isnan(c_buf[-pad:]).all()


def cuts(n, sizes, rng):
    out = []
    while sum(out) < n:
        out.append(min(int(rng.choice(sizes)), n - sum(out)))
    return out


def stream_run(st, x, f0, mode, seed, plain=True):
    rng = np.random.default_rng(seed)
    hop, span, (T, F) = st.hop, st.span, (x.shape[1], f0.shape[1])
    xs, fs = cuts(T, [0, 1, 1, hop, span // 2, span + 3, 3 * span + 1], rng), cuts(F, [0, 1, 2, 3, 10], rng)
    push = st.push_all if plain else st.push
    ev = [("x", n) for n in xs] + [("f", n) for n in fs]
    if mode == "mixed":
        ev = [ev[i] for i in rng.permutation(len(ev))]
    elif mode == "f0 first":
        ev = [("f", F)] + ev[:len(xs)]
    elif mode == "audio first":
        ev = [("x", T)] + ev[len(xs):]
    outs, px, pf = [], 0, 0
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

        assert all(isinstance(o, AudioTensor) and o.hop_length == hop for o in outs)
        outs = [(o.as_tensor(),) for o in outs]
    assert any(o[0].shape[1] == 0 for o in outs)
    return tuple(torch.cat([o[i] for o in outs], 1) for i in range(len(outs[0])))


@pytest.mark.parametrize("name", ["n64", "n256", "mixed", "T_short", "clamps", "n_ceps241"])
def test_stream_equals_the_module(name):
    from golf_amd.analysis_stream import SpectralEnvelopeStream, open_analysis_stream
    from golf_amd.envelope import SpectralEnvelopeAnalysis

    x, f0, kw = R.cases()[name]
    x, f0 = dev(x), dev(f0)
    order = kw["n_ceps"] - 1 if "n_ceps" in kw else None
    m = SpectralEnvelopeAnalysis(kw["sample_rate"], kw["hop"], kw["n_fft"], order, kw.get("f0_floor"), kw.get("f0_ceil"),
                                 kw.get("unvoiced_f0", 500.0))
    both, fwd = m.analyse(x, f0), m(x, f0).as_tensor()
    st = open_analysis_stream(m, x.shape[0])
    assert type(st) is SpectralEnvelopeStream and st.latency == hwmax_of(kw) + 1
    for mode, seed in (("mixed", 1), ("mixed", 2), ("f0 first", 3), ("audio first", 4)):   # one stream, utterance after utterance
        got = stream_run(st, x, f0, mode, seed)
        assert len(got) == 2 and all(torch.equal(g, w) for g, w in zip(got, both)), (name, mode)
    got = stream_run(st, x, f0, "mixed", 5, plain=False)      # push / finish: the type of forward
    assert len(got) == 1 and torch.equal(got[0], fwd)
    alone = stream_run(SpectralEnvelopeStream(m, 1), x[1:2], f0[1:2], "mixed", 6)
    assert all(torch.equal(a[0], w[1]) for a, w in zip(alone, both))
    assert [tuple(t.shape) for t in st.finish_all()] == [(x.shape[0], 0, both[0].shape[2]), (x.shape[0], 0, both[1].shape[2])]


def test_nhv_live_chain(golden):
    """F0TrackerStream(lag=8) -> SpectralEnvelopeStream + HarmonicNoiseStream -> HarmonicPlusNoiseStream on the shipped NHV
    decoder with fixed noise, B = 2, half a second in blocks of 0 to 3 600 samples, against the one-shot chain on the same
    fixed-lag f0 (the analyses' ``forward`` on the whole waveform -> the decoder): the controls are ``torch.equal``, and so is
    the audio."""
    import hna_ref
    from golf_amd.analysis_stream import F0TrackerStream, HarmonicNoiseStream, SpectralEnvelopeStream
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.envelope import SpectralEnvelopeAnalysis
    from golf_amd.f0 import F0Tracker
    from golf_amd.hna import HarmonicNoiseAnalysis
    from golf_amd.stream import HarmonicPlusNoiseStream, open_stream
    from test_gpu_stream_stft import _decoder, _fixed_noise, _inputs

    B, T, hop, sr = 2, 12000, 240, 24000.0
    F = T // hop + 1
    tr = [np.linspace(110.0, 160.0, F), 200.0 * 2 ** (0.03 * np.sin(0.4 * np.arange(F)))]
    x = torch.tensor(np.array([hna_ref.voice(t, T, 30, 900 + i) for i, t in enumerate(tr)]).astype(np.float32)).cuda()
    x[0, 5000:7000] = 0      # a silent stretch
    base = _inputs("nhv", B, T + 4 * hop)
    noise = base["noise"]
    dec = _decoder(golden, "nhv", base)
    dec.noise_generator = _fixed_noise(noise)
    order, n_mag = base["ctrl"].shape[2] - 1, base["log_mag"].shape[2]   # what the shipped decoder's two filters take
    tracker = F0Tracker(sr, hop).cuda()
    env = SpectralEnvelopeAnalysis(sr, hop, 1024, order)
    hna = HarmonicNoiseAnalysis(sr, hop, 8, n_mag=n_mag).cuda()

    def f0_fill(f0):   # the pulse train's equal-energy factor needs a positive f0: unvoiced frames sound at 100 Hz
        return torch.where(f0 > 0, f0, torch.full_like(f0, 100.0))

    def decode(st, f0, ceps, log_mag, nz):
        return st.push(phase=AudioTensor(f0_fill(f0) / sr, hop), harm_oscillator_params=(),
                       harm_filter_params=(AudioTensor(ceps, hop),), noise_filter_params=(AudioTensor(log_mag, hop),),
                       noise=AudioTensor(nz))

    # the one-shot chain on the fixed-lag f0
    f0_st = F0TrackerStream(tracker, B, lag=8)
    f0_all = torch.cat([f0_st.push(x).as_tensor(), f0_st.finish().as_tensor()], 1)
    assert f0_all.shape == (B, F) and (f0_all > 0).any() and (f0_all == 0).any()
    ceps_all, lm_all = env(x, f0_all).as_tensor(), hna(x, f0_all)[1].as_tensor()
    whole = open_stream(dec, B)
    assert type(whole) is HarmonicPlusNoiseStream
    y_ref = torch.cat([decode(whole, f0_all, ceps_all, lm_all, noise), whole.finish()], 1)

    # the live chain
    env_st, hna_st, out = SpectralEnvelopeStream(env, B), HarmonicNoiseStream(hna, B), open_stream(dec, B)
    f0s, cs, lms, ys, pos = [], [], [], [], 0
    for n in (2400, 1, 0, 2399, 3600, 3600):
        block, nz = x[:, pos:pos + n], noise[:, pos:pos + n]
        pos += n
        f0 = f0_st.push(block)
        c, lm = env_st.push(block, f0), hna_st.push(block, f0)[1]
        # the two analyses are final at different lags: the decoder stream takes each track at its own pace
        ys.append(decode(out, f0.as_tensor(), c.as_tensor(), lm.as_tensor(), nz))
        f0s.append(f0.as_tensor()), cs.append(c.as_tensor()), lms.append(lm.as_tensor())
    assert pos == T
    f0 = f0_st.finish()
    c = torch.cat([env_st.push(f0=f0).as_tensor(), env_st.finish().as_tensor()], 1)
    lm = torch.cat([hna_st.push(f0=f0)[1].as_tensor(), hna_st.finish()[1].as_tensor()], 1)
    f0s.append(f0.as_tensor()), cs.append(c), lms.append(lm)
    ys.append(decode(out, f0.as_tensor(), c, lm, noise[:, pos:]))
    ys.append(out.finish())
    assert torch.equal(torch.cat(f0s, 1), f0_all)
    assert torch.equal(torch.cat(cs, 1), ceps_all) and torch.equal(torch.cat(lms, 1), lm_all)
    assert sum(t.shape[1] > 0 for t in cs[:-1]) >= 3       # frames came out while the audio was still coming in
    y = torch.cat(ys, 1)
    assert y.shape == y_ref.shape and y.shape[1] > T - 3 * hop and torch.isfinite(y).all() and float(y.abs().max()) > 1e-3
    assert torch.equal(y, y_ref)
    with torch.no_grad():
        one = dec(phase=AudioTensor(f0_fill(f0_all) / sr, hop), harm_oscillator_params=(), noise_generator_params=(),
                  harm_filter_params=(AudioTensor(ceps_all, hop),), noise_filter_params=(AudioTensor(lm_all, hop),)).as_tensor()
    m = min(one.shape[1], y.shape[1])
    print("nhv live chain against the decoder's forward: max |diff|", float((y[:, :m] - one[:, :m]).abs().max()),
          "of", float(one.abs().max()), "shapes", tuple(y.shape), tuple(one.shape))
    assert y.shape == one.shape and torch.equal(y, one)
