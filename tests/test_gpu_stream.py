"""Streaming GOLF-ss synthesis on the device: the carried-state all-pole entry, the carried-phase oscillator and DecoderStream
against the one-shot decoder and the float64 oracle."""
import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu


def _splits(rng, total, step=1, max_len=None, zeros=True):
    """Random cut points of [0, total) on multiples of ``step`` (zero-length pieces included)."""
    out, pos = [], 0
    while pos < total:
        n = int(rng.integers(0, (max_len or total) // step + 1)) * step if zeros else 0
        n = min(max(n, 0), total - pos)
        out.append(n)
        pos += n
        if rng.random() < 0.1:
            out.append(0)
    return out


@pytest.mark.parametrize("B,M,hop,F", [(1, 22, 240, 12), (64, 22, 240, 12), (3, 7, 250, 9), (64, 7, 250, 9)])
def test_state_entry_vs_oracle(B, M, hop, F):
    """golf_ltv_allpole_fwd_state_f32 from a random state vs the float64 oracle with zi, the returned state = the last M
    outputs; a block shorter than M shifts the old state in."""
    from golf_amd import functional as GF
    from oracle import golf_oracle as O

    from golf_amd.synthetic import make_inputs

    rng = np.random.default_rng(B * 1000 + M)
    T = (F - 1) * hop
    inp = make_inputs(B=B, T=F * hop, hop=hop, M=M)
    x = inp["noise"][:, :T].numpy()
    gain, a = inp["gain"][:, :F].numpy(), inp["a"][:, :F].numpy()
    zi = rng.normal(0, 0.3, (B, M)).astype(np.float32)
    st = torch.tensor(zi).cuda()
    y = GF.ltv_allpole_ss_state(torch.tensor(x).cuda(), torch.tensor(gain).cuda(), torch.tensor(a).cuda(), hop, st)
    torch.cuda.synchronize()
    A = np.stack([np.asarray(GF.linear_upsample(torch.tensor(a[..., i]).double(), hop))[:, :T] for i in range(M)], -1)
    G = np.asarray(GF.linear_upsample(torch.tensor(gain).double(), hop))[:, :T]
    ref = O.sample_wise_lpc(x.astype(np.float64) * G, A, zi.astype(np.float64))
    emax, el2 = rel_err(y.cpu().numpy(), ref)
    assert emax < 1e-4 and el2 < 1e-4, (emax, el2)
    np.testing.assert_array_equal(st.cpu().numpy(), y.cpu().numpy()[:, ::-1][:, :M])
    # a block shorter than M: y[-1-i] for i < T, then the old state shifted by T
    Ts = 3
    st2 = torch.tensor(zi).cuda()
    y2 = GF.ltv_allpole_ss_state(torch.tensor(x[:, :Ts]).cuda(), torch.tensor(gain[:, :2]).cuda(), torch.tensor(a[:, :2]).cuda(),
                                 hop, st2)
    expect = np.concatenate([y2.cpu().numpy()[:, ::-1], zi[:, : M - Ts]], 1)
    np.testing.assert_array_equal(st2.cpu().numpy(), expect)


@pytest.mark.parametrize("B,M,hop", [(1, 22, 240), (32, 22, 240), (64, 22, 240), (5, 7, 250)])
def test_allpole_split_invariance_bitwise(B, M, hop):
    """Frame-aligned blocks chained through the state give the bits of the one-shot serial filter (last sample included)."""
    from golf_amd import functional as GF
    from golf_amd.synthetic import make_inputs

    F = 40
    inp = make_inputs(B=B, T=F * hop, hop=hop, M=M, device="cuda")
    gain, a = inp["gain"][:, :F].contiguous(), inp["a"][:, :F].contiguous()
    T = (F - 1) * hop + 1
    x = inp["noise"][:, :T].contiguous()
    whole = GF.ltv_allpole_ss(x, gain, a, hop, mode="serial")
    rng = np.random.default_rng(B + M)
    st = torch.zeros(B, M, device="cuda")
    cuts = np.sort(rng.choice(np.arange(1, F - 1), size=6, replace=False))
    bounds = [0] + list(cuts) + [F - 1]
    parts = []
    for f0, f1 in zip(bounds[:-1], bounds[1:]):
        hi = f1 * hop + (1 if f1 == F - 1 else 0)
        parts.append(GF.ltv_allpole_ss_state(x[:, f0 * hop: hi], gain[:, f0: f1 + 1], a[:, f0: f1 + 1], hop, st))
    got = torch.cat(parts, 1)
    assert torch.equal(got, whole)


def test_oscillator_random_splits():
    """The carried-phase oscillator over random splits: wrapped phase bit-identical to the one-shot accumulation; decimated
    output within 1e-6 of the fused oscillator and 1e-4 of the float64 oracle."""
    from golf_amd import functional as GF
    from golf_amd.synthetic import make_decoder, make_inputs
    from oracle import golf_oracle as O

    B = 4
    inp = make_inputs(B=B, T=24000, device="cuda")
    osc = make_decoder(noise_filter=False, room_filter=False).harm_oscillator.cuda()
    table, taps = osc.table, osc.decimater.taps
    phase, wsel, w_hop = inp["phase"], inp["wsel"], inp["w_hop"]
    Tp = phase.shape[1]
    rng = np.random.default_rng(5)
    acc = torch.zeros(B, dtype=torch.int64, device="cuda")
    pres, wraps, j = [], [], 0
    for n in _splits(rng, Tp - 1, max_len=3000):
        if n == 0:
            continue
        p, w = GF.glottal_osc_stream(phase[:, j: j + n + 1], j, n, False, 1, 4, wsel, 0, w_hop, table, True, acc,
                                     want_wrapped=True)
        pres.append(p)
        wraps.append(w)
        j += n
    p, w = GF.glottal_osc_stream(phase[:, j: j + 1], j, 0, True, 1, 4, wsel, 0, w_hop, table, True, acc, want_wrapped=True)
    pres.append(p)
    wraps.append(w)
    pre, wrapped = torch.cat(pres, 1), torch.cat(wraps, 1)
    one_wrapped, _ = GF.instantaneous_phase(phase, 1, 4)
    assert torch.equal(wrapped, one_wrapped)
    out = GF.decimate_fir(pre, taps, 4)
    fused = GF.glottal_osc(phase, wsel, table, taps, 1, w_hop, 4, True)
    emax, _ = rel_err(out.cpu().numpy(), fused.cpu().numpy())
    assert emax < 1e-6, emax
    ref = O.indexed_glottal_forward(phase.cpu().numpy(), 1, wsel.cpu().numpy(), w_hop, table.cpu().numpy(), 4, True,
                                    decim_taps=taps.cpu().numpy())["out"]
    emax, el2 = rel_err(out.cpu().numpy(), ref)
    assert emax < 1e-4 and el2 < 1e-4


def _push_random(st, inp, rng, with_fir=True, noise=True, cast=None):
    """Push every track in independent random slices (0, 1, < M and off-frame lengths included), then finish."""
    from golf_amd.audiotensor import AudioTensor

    c = cast if cast is not None else (lambda t: t)
    tracks = dict(phase=(inp["phase"], 1), wsel=(inp["wsel"], inp["w_hop"]), gain=(inp["gain"], 240), a=(inp["a"], 240))
    if with_fir:
        tracks["log_mag"] = (inp["log_mag"], 240)
    if noise:
        tracks["noise"] = (inp["noise"], 1)
    pos = {k: 0 for k in tracks}
    outs = []
    choices = {1: [0, 1, 7, 17, 240, 333, 2400, 4801], 240: [0, 1, 2, 3, 11], 2400: [0, 1, 2]}
    while any(pos[k] < v[0].shape[1] for k, v in tracks.items()):
        sl = {}
        for k, (t, hop) in tracks.items():
            n = int(rng.choice(choices[1 if hop == 1 else (240 if hop == 240 else 2400)]))
            sl[k] = AudioTensor(t[:, pos[k]: pos[k] + n], hop)
            pos[k] = min(pos[k] + n, t.shape[1])
        outs.append(st.push(phase=sl["phase"],
                            harm_oscillator_params=(AudioTensor(c(sl["wsel"].as_tensor()), inp["w_hop"]),),
                            noise_filter_params=(AudioTensor(c(sl["log_mag"].as_tensor()), 240),) if with_fir else (),
                            end_filter_params=(AudioTensor(c(sl["gain"].as_tensor()), 240),
                                               AudioTensor(c(sl["a"].as_tensor()), 240)),
                            noise=sl.get("noise")))
        assert outs[-1].shape[1] % 240 == 0
    outs.append(st.finish())
    return torch.cat(outs, 1)


def test_full_decoder_stream_vs_one_shot_and_oracle():
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.stream import DecoderStream
    from golf_amd.synthetic import make_decoder, make_inputs
    from oracle import golf_oracle as O

    inp = make_inputs(B=32, device="cuda", with_noise_filter=True)
    dec = make_decoder(noise_filter=True, room_filter=True, injected_noise=inp["noise"]).cuda()
    with torch.no_grad():
        dec.room_filter.kernel.copy_(inp["room_kernel"])
        one = dec(phase=AudioTensor(inp["phase"]), harm_oscillator_params=(AudioTensor(inp["wsel"], inp["w_hop"]),),
                  noise_generator_params=(), noise_filter_params=(AudioTensor(inp["log_mag"], 240),),
                  end_filter_params=(AudioTensor(inp["gain"], 240), AudioTensor(inp["a"], 240))).as_tensor()
    st = DecoderStream(dec, batch_size=32)
    y = _push_random(st, inp, np.random.default_rng(11))
    assert st.latency == 2655
    assert y.shape == (32, 47760) == one.shape
    emax, _ = rel_err(y.cpu().numpy(), one.cpu().numpy())
    assert emax < 2e-4, emax
    nb = 2
    c = lambda k: inp[k][:nb].double().cpu().numpy()
    osc = dec.harm_oscillator
    win = torch.hann_window(510, dtype=torch.float64).numpy()
    _, ref = O.golf_ss_decoder(c("phase"), 1, c("wsel"), inp["w_hop"], osc.table.double().cpu().numpy(), c("noise"),
                               c("log_mag"), win, c("gain"), c("a"), 240,
                               room_kernel=inp["room_kernel"].double().cpu().numpy(), oversampling=4,
                               equal_energy=True, decim_taps=osc.decimater.kernel.double().cpu().numpy().ravel())
    emax, el2 = rel_err(y[:nb].cpu().numpy(), ref)
    assert emax < 1e-4 and el2 < 1e-4, (emax, el2)


def test_stream_without_noise_filter_keeps_the_last_sample():
    """PassThrough noise filter: the one-shot filters (F-1)*hop + 1 samples; the stream's last sample (alone in its frame)
    carries the same bits as the serial one-shot's."""
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.stream import DecoderStream
    from golf_amd.synthetic import make_decoder, make_inputs

    inp = make_inputs(B=4, T=12000, device="cuda")
    dec = make_decoder(noise_filter=False, room_filter=False, injected_noise=inp["noise"]).cuda()
    with torch.no_grad():
        one = dec(phase=AudioTensor(inp["phase"]), harm_oscillator_params=(AudioTensor(inp["wsel"], inp["w_hop"]),),
                  noise_generator_params=(), noise_filter_params=(),
                  end_filter_params=(AudioTensor(inp["gain"], 240), AudioTensor(inp["a"], 240))).as_tensor()
    st = DecoderStream(dec, batch_size=4)
    y = _push_random(st, inp, np.random.default_rng(3), with_fir=False)
    assert y.shape == one.shape == (4, (inp["a"].shape[1] - 1) * 240 + 1)
    emax, _ = rel_err(y.cpu().numpy(), one.cpu().numpy())
    assert emax < 2e-4, emax


def test_generated_noise_and_autocast_bf16(golden):
    """The golf-ss decoder built from the shipped config: a stream that draws its own noise runs under bf16 autocast with
    bf16 control tracks (the phase stays fp32: it is accumulated over the utterance) and matches fp32 streaming of the same
    values (same noise) to the bound of the existing autocast test."""
    from golf_amd.config import build_model
    from golf_amd.stream import DecoderStream
    from golf_amd.synthetic import make_inputs

    g = golden("g28_shipped_configs")
    paths = list(g["path"])
    rel = "ckpts/interspeech24/golf-ss/config.yaml"
    dec = getattr(build_model(str(g["config"][paths.index(rel)])), "decoder").cuda().eval()
    inp = make_inputs(B=2, T=12000, device="cuda", with_noise_filter=True)
    torch.manual_seed(0)
    st = DecoderStream(dec, batch_size=2)
    y32 = _push_random(st, inp, np.random.default_rng(1), noise=False, cast=lambda t: t.to(torch.bfloat16).float())
    torch.manual_seed(0)
    st = DecoderStream(dec, batch_size=2)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y16 = _push_random(st, inp, np.random.default_rng(1), noise=False, cast=lambda t: t.to(torch.bfloat16))
    assert y16.dtype == torch.float32 and y16.shape == y32.shape
    assert torch.isfinite(y16).all()
    _, el2 = rel_err(y16.cpu().numpy(), y32.cpu().numpy())
    assert el2 < 5e-2, el2
