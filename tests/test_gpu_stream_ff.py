"""Streaming frame-wise synthesis on the device: golf_lti_frames_ola_stream_f32 against the float64 oracle and the one-shot
entry (split invariance bit for bit), and FramewiseDecoderStream for golf-ff and golf-v1 against the one-shot decoders and the
oracle composition."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from test_stream_ff_host import _compose

pytestmark = pytest.mark.gpu


def _win(W):
    return torch.hann_window(W).cuda()


def _stream_filter(ex, gain, a, win, hop, cuts):
    """Drive the streaming entry over frame chunks ``cuts`` (chunk sizes in frames, 0 included), each call given exactly the
    windows its frames read, then finish; returns the concatenated output."""
    from golf_amd import functional as GF

    B, T0 = ex.shape
    F, W = a.shape[1], win.numel()
    Tx, nfr, Ty = GF.ff_output_length(T0, F, hop, W)
    pad = W // 2
    seg = lambda t, fin: min(t // hop, F - 2) if fin else t // hop
    # while open, frame f needs all of x[.., f*hop - pad + W) and the gain rows up to its last sample's segment + 1
    f_open = min((Tx + pad - W) // hop + 1, F - 1 - (W - pad - 1) // hop)
    outs, carry, f0, n0 = [], None, 0, 0
    bounds = list(np.cumsum(cuts))
    for i, f1 in enumerate(bounds + [nfr]):
        fin = i == len(bounds)
        f1 = max(f0, min(int(f1), nfr if fin else f_open))
        nf = f1 - f0
        ny = (Ty if fin else max(0, f1 * hop - pad)) - n0
        tlo = max(0, f0 * hop - pad)
        thi = (f1 - 1) * hop - pad + W if nf else tlo
        thi = min(thi, Tx) if fin else thi
        thi = max(thi, tlo)
        g_lo = seg(tlo, fin) if nf else 0
        g_hi = seg(thi - 1, fin) + 2 if thi > tlo else g_lo
        y, carry = GF.lti_frames_ola_stream(ex[:, tlo:thi], gain[:, g_lo:g_hi], a[:, f0:f0 + nf], win, hop, carry, x0=tlo,
                                            g0=g_lo, a0=f0, f0=f0, nf=nf, n0=n0, ny=ny, x_end=Tx if fin else -1,
                                            g_end=F if fin else -1)
        outs.append(y)
        f0, n0 = f0 + nf, n0 + ny
    return torch.cat(outs, 1)


def _random_cuts(rng, n):
    cuts, tot = [], 0
    while tot < n:
        c = int(rng.choice([0, 1, 1, 2, 3, 7, 20]))
        cuts.append(c)
        tot += c
    return cuts


@pytest.mark.parametrize("B,M,hop,W", [(1, 22, 240, 960), (64, 22, 240, 960), (3, 22, 240, 480), (5, 7, 250, 1000)])
def test_stream_entry_vs_oracle_one_shot_and_splits(B, M, hop, W):
    """Against the float64 oracle (rel-max / rel-l2 <= 1e-4) and the one-shot entry (<= 2e-4); random splits, zero-length
    calls included, give the bits of one call over the whole.  (hop 250: not a multiple of 4 -- the direct-form kernel.)"""
    from golf_amd import functional as GF
    from golf_amd.synthetic import make_inputs
    from oracle import golf_oracle as O

    F = 40
    inp = make_inputs(B=B, T=F * hop, hop=hop, M=M, device="cuda")
    gain, a = inp["gain"][:, :F].contiguous(), inp["a"][:, :F].contiguous()
    ex = inp["noise"][:, :(F - 1) * hop + 1].contiguous()
    win = _win(W)
    nfr = GF.ff_output_length(ex.shape[1], F, hop, W)[1]
    whole = _stream_filter(ex, gain, a, win, hop, [])
    ref, _ = O.lti_frames_ola_forward(ex.double().cpu().numpy(), gain.double().cpu().numpy(), a.double().cpu().numpy(), hop,
                                      win.double().cpu().numpy())
    emax, el2 = rel_err(whole.cpu().numpy(), ref)
    assert emax <= 1e-4 and el2 <= 1e-4, (emax, el2)
    one = GF.lti_frames_ola(ex, gain, a, win, hop)
    assert one.shape == whole.shape
    emax, _ = rel_err(whole.cpu().numpy(), one.cpu().numpy())
    assert emax <= 2e-4, emax
    rng = np.random.default_rng(B * 100 + hop)
    for _ in range(3):
        got = _stream_filter(ex, gain, a, win, hop, _random_cuts(rng, nfr))
        assert torch.equal(got, whole)


def test_one_frame_calls_wrap_the_ring():
    """B 2, M 6, hop 8, W 32 (S = 3): one frame per call up to frame 11, so the slots the carried frames are read from and
    written to wrap more than once; the bits of one call over the whole."""
    from golf_amd import functional as GF

    B, M, hop, W, F = 2, 6, 8, 32, 14
    gen = torch.Generator().manual_seed(832)
    a = GF.rc2lpc((0.5 * torch.tanh(torch.randn(B, F, M, generator=gen))).cuda())
    gain = torch.exp(0.1 * torch.randn(B, F, generator=gen)).cuda()
    ex = torch.randn(B, (F - 1) * hop + 1, generator=gen).cuda()
    whole = _stream_filter(ex, gain, a, _win(W), hop, [])
    got = _stream_filter(ex, gain, a, _win(W), hop, [1] * 12)
    assert whole.shape[1] == (F - 1) * hop and whole.abs().max() > 0.1
    assert torch.equal(got, whole)


def test_stream_ill_conditioned_rows():
    """tests/test_gpu_lpc_ff.py::test_ff_ill_conditioned_rows through the streaming entry (random splits): the same bound,
    worst row <= 3e-4 and the second worst <= 1e-4 -- the per-frame fp64 feedback tier keeps the hard frames accurate."""
    from oracle import golf_oracle as O

    rng = np.random.default_rng(40)
    B, F, M, hop, W = 48, 200, 22, 240, 960
    logits = rng.normal(0, 0.5, (B, 1, M)) + np.cumsum(rng.normal(0, 0.02, (B, F, M)), 1)
    a = O.rc2lpc(np.tanh(logits)).astype(np.float32)[:32]
    gain = np.exp(-3 + np.cumsum(rng.normal(0, 0.05, (B, F)), 1)).astype(np.float32)[:32]
    ex = rng.normal(0, 1, (B, (F - 1) * hop + 1)).astype(np.float32)[:32]
    win = torch.hann_window(W).double().numpy()
    ref, _ = O.lti_frames_ola_forward(ex, gain, a, hop, win, centred=True)
    t = lambda v: torch.tensor(v).cuda()
    y = _stream_filter(t(ex), t(gain), t(a), _win(W), hop, _random_cuts(np.random.default_rng(3), 199)).cpu().numpy()
    err = np.abs(y - ref).max(1) / np.abs(ref).max(1)
    print("worst rows", np.argsort(err)[-3:], np.sort(err)[-3:])
    assert err.max() <= 3e-4 and np.sort(err)[-2] <= 1e-4, (int(err.argmax()), float(err.max()))


def _push_random(st, inp, rng, lpc_key, noise=True, cast=None):
    """Every track in independent random slices (0, 1 and off-frame lengths included), then finish()."""
    from golf_amd.audiotensor import AudioTensor

    c = cast if cast is not None else (lambda t: t)
    tracks = dict(phase=(inp["phase"], 1), wsel=(inp["wsel"], inp["w_hop"]), gain=(inp["gain"], 240), a=(inp["a"], 240),
                  log_mag=(inp["log_mag"], 240))
    if noise:
        tracks["noise"] = (inp["noise"], 1)
    pos = {k: 0 for k in tracks}
    outs = []
    choices = {1: [0, 1, 7, 17, 240, 333, 2400, 4801], 240: [0, 1, 2, 3, 11], 2400: [0, 1, 2]}
    while any(pos[k] < v[0].shape[1] for k, v in tracks.items()):
        sl = {}
        for k, (t, hop) in tracks.items():
            n = int(rng.choice(choices[1 if hop == 1 else (240 if hop == 240 else 2400)]))
            sl[k] = t[:, pos[k]: pos[k] + n]
            pos[k] = min(pos[k] + n, t.shape[1])
        lpc = (AudioTensor(c(sl["gain"]), 240), AudioTensor(c(sl["a"]), 240))
        outs.append(st.push(phase=AudioTensor(sl["phase"]), harm_oscillator_params=(AudioTensor(c(sl["wsel"]), inp["w_hop"]),),
                            noise_filter_params=(AudioTensor(c(sl["log_mag"]), 240),), **{lpc_key: lpc},
                            noise=AudioTensor(sl["noise"]) if "noise" in sl else None))
    outs.append(st.finish())
    return torch.cat(outs, 1)


def _fixed_noise(noise):
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.noise import NoiseInterface

    class Fixed(NoiseInterface):
        uses_reference_values = False

        def forward(self, ref, *args, **kwargs):
            return AudioTensor(noise[:, : ref.shape[1]])

    return Fixed()


def _shipped(golden, rel):
    from golf_amd.config import build_model

    g = golden("g28_shipped_configs")
    paths = list(g["path"])
    return getattr(build_model(str(g["config"][paths.index(rel)])), "decoder").cuda().eval()


def _check_decoder(dec, inp, hpn, seed):
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.stream import FramewiseDecoderStream, open_stream

    lpc_key = "harm_filter_params" if hpn else "end_filter_params"
    lpc = (AudioTensor(inp["gain"], 240), AudioTensor(inp["a"], 240))
    with torch.no_grad():
        one = dec(phase=AudioTensor(inp["phase"]), harm_oscillator_params=(AudioTensor(inp["wsel"], inp["w_hop"]),),
                  noise_generator_params=(), noise_filter_params=(AudioTensor(inp["log_mag"], 240),),
                  **{lpc_key: lpc}).as_tensor()
    B = inp["phase"].shape[0]
    st = open_stream(dec, B)
    assert isinstance(st, FramewiseDecoderStream)
    y = _push_random(st, inp, np.random.default_rng(seed), lpc_key)
    assert st.latency == 3375
    assert y.shape == one.shape, (y.shape, one.shape)
    emax, _ = rel_err(y.cpu().numpy(), one.cpu().numpy())
    assert emax <= 2e-4, emax
    nb = 2
    osc = dec.harm_oscillator
    c = lambda k: inp[k][:nb].double().cpu().numpy()
    ref = _compose(dict({k: c(k) for k in ("phase", "wsel", "noise", "log_mag", "gain", "a")}, w_hop=inp["w_hop"],
                        room_kernel=inp["room_kernel"].double().cpu().numpy()),
                   osc.table.double().cpu().numpy(), osc.decimater.taps.double().cpu().numpy(), hpn)
    emax, el2 = rel_err(y[:nb].cpu().numpy(), ref)
    assert emax <= 1e-4 and el2 <= 1e-4, (emax, el2)
    # a second random split: the same bits (every frame is filtered once, its tier decided by its own coefficients)
    y2 = _push_random(open_stream(dec, B), inp, np.random.default_rng(seed + 1), lpc_key)
    assert torch.equal(y, y2)


def test_golf_ff_decoder_stream_vs_one_shot_and_oracle():
    from golf_amd.synthetic import make_decoder, make_inputs

    inp = make_inputs(B=32, device="cuda", with_noise_filter=True)
    dec = make_decoder(noise_filter=True, room_filter=True, injected_noise=inp["noise"], framewise=True).cuda()
    with torch.no_grad():
        dec.room_filter.kernel.copy_(inp["room_kernel"])
    _check_decoder(dec, inp, hpn=False, seed=11)


def test_golf_v1_shipped_config_stream_vs_one_shot_and_oracle(golden):
    from golf_amd.synthetic import make_inputs

    inp = make_inputs(B=32, device="cuda", with_noise_filter=True)
    dec = _shipped(golden, "ckpts/interspeech24/golf-v1/config.yaml")
    dec.noise_generator = _fixed_noise(inp["noise"])
    with torch.no_grad():
        dec.end_filter.kernel.copy_(inp["room_kernel"])
    _check_decoder(dec, inp, hpn=True, seed=12)


def test_golf_ff_generated_noise_and_autocast_bf16(golden):
    """golf-ff from the shipped config drawing its own noise, under bf16 autocast with bf16 control tracks, against fp32
    streaming of the same values and noise (the bound of tests/test_gpu_stream.py's autocast test)."""
    from golf_amd.stream import FramewiseDecoderStream
    from golf_amd.synthetic import make_inputs

    dec = _shipped(golden, "ckpts/interspeech24/golf-ff/config.yaml")
    inp = make_inputs(B=2, T=12000, device="cuda", with_noise_filter=True)
    bf = lambda t: t.to(torch.bfloat16)
    torch.manual_seed(0)
    y32 = _push_random(FramewiseDecoderStream(dec, 2), inp, np.random.default_rng(1), "end_filter_params", noise=False,
                       cast=lambda t: bf(t).float())
    torch.manual_seed(0)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y16 = _push_random(FramewiseDecoderStream(dec, 2), inp, np.random.default_rng(1), "end_filter_params", noise=False,
                           cast=bf)
    assert y16.dtype == torch.float32 and y16.shape == y32.shape
    assert torch.isfinite(y16).all()
    _, el2 = rel_err(y16.cpu().numpy(), y32.cpu().numpy())
    assert el2 < 5e-2, el2
