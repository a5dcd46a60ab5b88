"""GPU: the glottal-source analysis block by block (analysis_stream.GlottalSourceStream) against the module's ``analyse`` on
the cases of tests/glottal_ref.py (tests/test_gpu_glottal.py pins those against the float64 restatement), whatever the cuts;
and the GOLF-ss live loop, LPCAnalysisStream -> ResidualStream -> GlottalSourceStream (+ F0TrackerStream) -> DecoderStream."""
import numpy as np
import pytest
import torch

import glottal_ref as R

pytestmark = pytest.mark.gpu


def dev(a):
    return a if isinstance(a, torch.Tensor) else torch.tensor(a).cuda()


def cuts(n, sizes, rng):
    out = []
    while sum(out) < n:
        out.append(min(int(rng.choice(sizes)), n - sum(out)))
    return out


def stream_run(st, e, f0, mode, seed, plain=True):
    """Push (e, f0) through ``st`` in seeded random cuts of each, finish, and concatenate: ``mixed`` interleaves the two at
    random, ``late`` delivers a frame's f0 eight frames after its last sample, ``f0 first`` / ``audio first`` deliver one input
    whole before the other starts."""
    rng = np.random.default_rng(seed)
    hop, span, (T, F) = st.hop, st.span, (e.shape[1], f0.shape[1])
    xs, fs = cuts(T, [0, 1, 1, hop, span // 2, span + 3, 3 * span + 1], rng), cuts(F, [0, 1, 2, 3, 10], rng)
    push = st.push_all if plain else st.push
    outs, px, pf = [], 0, 0
    if mode == "late":
        for n in xs:
            k = max(min((px + n) // hop - 8, F) - pf, 0)
            outs.append(push(e[:, px:px + n], f0[:, pf:pf + k]))
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
                outs.append(push(e=e[:, px:px + n]))
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


@pytest.mark.parametrize("name", list(R.cases()))
def test_stream_equals_the_module(name):
    from golf_amd.analysis_stream import GlottalSourceStream, open_analysis_stream
    from golf_amd.glottal import GlottalSourceAnalysis

    c = R.cases()[name]
    e, f0 = dev(c["x"]), dev(c["f0"])
    m = GlottalSourceAnalysis(dev(c["table"]), c["sample_rate"], c["hop"], num_harmonics=c["H"], n_phi=c["n_phi"],
                              unvoiced_weight=0.25).cuda()
    three = m.analyse(e, f0)
    assert all(torch.isfinite(t).all() for t in three)
    st = open_analysis_stream(m, e.shape[0])
    assert type(st) is GlottalSourceStream and st.span == max(2048, 4 * c["hop"]) and st.latency == st.span - st.span // 2
    for mode, seed in (("mixed", 1), ("late", 2), ("f0 first", 3), ("audio first", 4)):   # one stream, utterance after utterance
        got = stream_run(st, e, f0, mode, seed)
        assert len(got) == 3 and all(torch.equal(g, w) for g, w in zip(got, three)), (name, mode)
    got = stream_run(st, e, f0, "mixed", 5, plain=False)      # push / finish: the type of forward
    assert len(got) == 1 and torch.equal(got[0], m(e, f0).as_tensor())
    alone = stream_run(GlottalSourceStream(m, 1), e[-1:], f0[-1:], "late", 6)
    assert all(torch.equal(a[0], w[-1]) for a, w in zip(alone, three))
    assert [tuple(t.shape) for t in st.finish_all()] == [(e.shape[0], 0)] * 3


def test_golf_ss_live_chain():
    """LPCAnalysisStream -> ResidualStream -> GlottalSourceStream, with F0TrackerStream(lag=8), -> DecoderStream on the GOLF-ss
    decoder with fixed noise, B = 2, half a second, block by block, against the same modules one-shot on the same fixed-lag
    f0 (LPCAnalysis -> residual_fused -> GlottalSourceAnalysis.analyse -> the decoder's stream given everything in one push):
    the controls and the audio are ``torch.equal``."""
    import hna_ref
    from conftest import rel_err
    from golf_amd.analysis_stream import F0TrackerStream, GlottalSourceStream, LPCAnalysisStream, ResidualStream
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.f0 import F0Tracker
    from golf_amd.glottal import GlottalSourceAnalysis
    from golf_amd.lpc import LPCAnalysis
    from golf_amd.stream import DecoderStream
    from golf_amd.synthetic import make_decoder

    B, T, hop, sr, M = 2, 12000, 240, 24000.0, 22
    F = T // hop + 1
    tr = [np.linspace(110.0, 160.0, F), 200.0 * 2 ** (0.03 * np.sin(0.4 * np.arange(F)))]
    x = torch.tensor(np.array([hna_ref.voice(t, T, 30, 800 + i) for i, t in enumerate(tr)]).astype(np.float32)).cuda()
    x = x + 1e-3 * torch.randn(B, T, generator=torch.Generator().manual_seed(6)).cuda()   # no frame is numerically singular
    x[0, 5000:7000] *= 1e-3      # a quiet stretch
    noise = 0.01 * torch.randn(B, T + 4 * hop, generator=torch.Generator().manual_seed(4)).cuda()
    dec = make_decoder(noise_filter=False, room_filter=False, injected_noise=noise).cuda().eval()
    lpc, tracker = LPCAnalysis(M, hop).cuda(), F0Tracker(sr, hop).cuda()
    glo = GlottalSourceAnalysis(dec.harm_oscillator, sr, hop).cuda()

    def f0_fill(f0):   # the oscillator needs a positive f0: unvoiced frames run at 100 Hz
        return torch.where(f0 > 0, f0, torch.full_like(f0, 100.0))

    def decode(st, f0, w, gain, a, nz):
        return st.push(phase=AudioTensor(f0_fill(f0) / sr, hop), harm_oscillator_params=(AudioTensor(w, hop),),
                       end_filter_params=(AudioTensor(gain, hop), AudioTensor(a, hop)), noise=AudioTensor(nz))

    # the modules one-shot, on the fixed-lag f0
    f0_st = F0TrackerStream(tracker, B, lag=8)
    f0_all = torch.cat([f0_st.push(x).as_tensor(), f0_st.finish().as_tensor()], 1)
    gain_all, a_all = lpc.analyse(x)
    assert f0_all.shape == gain_all.shape == (B, F) and (f0_all > 0).any()
    e_all = glo.residual_fused(x, gain_all, a_all)
    assert e_all.shape == (B, T) and torch.isfinite(e_all).all()
    w_all = glo.analyse(e_all, f0_all)[0]
    whole = DecoderStream(dec, B)
    y_ref = torch.cat([decode(whole, f0_all, w_all, gain_all, a_all, noise), whole.finish()], 1)

    # the live chain
    lpc_st, res_st, glo_st, out = LPCAnalysisStream(lpc, B), ResidualStream(hop, M, B), GlottalSourceStream(glo, B), \
        DecoderStream(dec, B)
    assert res_st.latency + lpc_st.latency == 240 + 480
    f0s, gs, es, ws, ys, pos = [], [], [], [], [], 0
    for n in (2400, 1, 0, 2399, 3000, 600, 3600):
        block, nz = x[:, pos:pos + n], noise[:, pos:pos + n]
        pos += n
        gain, a = lpc_st.push(block)
        e = res_st.push(block, gain, a)
        f0 = f0_st.push(block)
        w = glo_st.push(e, f0)
        ys.append(decode(out, f0.as_tensor(), w.as_tensor(), gain.as_tensor(), a.as_tensor(), nz))
        f0s.append(f0.as_tensor()), gs.append(gain.as_tensor()), es.append(e), ws.append(w.as_tensor())
    assert pos == T
    gain, a = lpc_st.finish()
    e = torch.cat([res_st.push(gain=gain, a=a), res_st.finish()], 1)
    f0 = f0_st.finish()
    w = torch.cat([glo_st.push(e, f0).as_tensor(), glo_st.finish().as_tensor()], 1)
    f0s.append(f0.as_tensor()), gs.append(gain.as_tensor()), es.append(e), ws.append(w)
    ys.append(decode(out, f0.as_tensor(), w, gain.as_tensor(), a.as_tensor(), noise[:, pos:]))
    ys.append(out.finish())
    assert torch.equal(torch.cat(f0s, 1), f0_all) and torch.equal(torch.cat(gs, 1), gain_all)
    assert torch.equal(torch.cat(es, 1), e_all) and torch.equal(torch.cat(ws, 1), w_all)
    assert sum(t.shape[1] > 0 for t in ws[:-1]) >= 3 and sum(t.shape[1] > 0 for t in es[:-1]) >= 4   # while the audio was coming in
    y = torch.cat(ys, 1)
    assert y.shape == y_ref.shape and y.shape[1] > T - 2 * hop and torch.isfinite(y).all() and float(y.abs().max()) > 1e-3
    assert torch.equal(y, y_ref)
    with torch.no_grad():
        one = dec(phase=AudioTensor(f0_fill(f0_all) / sr, hop), harm_oscillator_params=(AudioTensor(w_all, hop),),
                  noise_generator_params=(), noise_filter_params=(),
                  end_filter_params=(AudioTensor(gain_all, hop), AudioTensor(a_all, hop))).as_tensor()
    emax, _ = rel_err(y.cpu().numpy(), one.cpu().numpy())
    print("golf-ss live chain against the decoder's forward: rel-max", emax)
    assert y.shape == one.shape and emax < 2e-4   # the decoder stream's own bound against forward (tests/test_gpu_stream.py)
