"""Device time per push and the real-time factor of streaming synthesis, beside the one-shot decoder on the same audio.
Needs a GPU; run under a time limit, e.g.  timeout -k 10 600 python tools/time_stream.py [--decoder golf-ff]

--decoder golf-ss (default: DecoderStream), golf-ff (FramewiseDecoderStream, the frame-wise end filter) or golf-v1
(FramewiseDecoderStream over HarmonicPlusNoiseSynth: the frame-wise filter on the oscillator, the room filter last);
ddsp, sawsing, pulse or glottal_d (HarmonicPlusNoiseStream over the decoders of the shipped configs in
tests/golden/g28_shipped_configs.npz, with the inputs tests/test_stream_hpn_host.py builds: DDSP at hop 240 with a per-sample
phase, the ISMIR'23 models at hop 120 with the phase and voicing at hop 120; pushes of one hop at B=1).

For B in {1, 32} and pushes of 240 and 2400 samples (every track sliced to the same stretch of time), 2 s utterances:
  push_us     mean device time of one push (CUDA events around the push, synchronised per push: the host side is included)
  rtf         device time of the whole stream / audio duration (24 kHz)
  oneshot_us  device time of one decoder(...) call on the whole utterance, and its rtf
One JSON line per configuration."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from golf_amd.audiotensor import AudioTensor  # noqa: E402
from golf_amd.stream import DecoderStream, FramewiseDecoderStream, HarmonicPlusNoiseStream  # noqa: E402
from golf_amd.synthetic import make_decoder, make_inputs  # noqa: E402

SR = 24000


def make_v1(noise):
    """golf-v1 as cfg/ae/decoder/golf-v1.yaml builds it, from make_decoder's oscillator, noise and filters."""
    from golf_amd.sf import HarmonicPlusNoiseSynth

    ff = make_decoder(noise_filter=True, room_filter=True, injected_noise=noise, framewise=True)
    return HarmonicPlusNoiseSynth(harm_oscillator=ff.harm_oscillator, noise_generator=ff.noise_generator,
                                  harm_filter=ff.end_filter, noise_filter=ff.noise_filter, end_filter=ff.room_filter)


HPN = ("ddsp", "sawsing", "pulse", "glottal_d")


def _time_stream(make_stream, args, T, push, reps):
    """Push [lo, lo + push) of every track until T, then finish(): per-push device times, total, samples out."""
    for _ in range(reps):
        st = make_stream()
        times, n_out = [], 0
        for lo in range(0, T, push):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            y = st.push(**args(lo, min(lo + push, T)))
            e.record()
            e.synchronize()
            times.append(s.elapsed_time(e) * 1e3)
            n_out += y.shape[1]
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        n_out += st.finish().shape[1]
        e.record()
        e.synchronize()
        total = sum(times) + s.elapsed_time(e) * 1e3
    return times, total, n_out


def _hpn_case(B: int, T: int, decoder: str):
    """(stream factory, push arguments of [lo, hi), one-shot call) over a shipped harmonic-plus-noise decoder."""
    import numpy as np

    tests = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
    sys.path.insert(0, tests)
    from test_stream_hpn_host import SPECS, make_hpn_inputs, shipped
    from test_gpu_stream_hpn import _call_args, _fixed_noise

    golden = lambda name: np.load(os.path.join(tests, "golden", name + ".npz"), allow_pickle=False)
    x = make_hpn_inputs(decoder, B, T, device="cuda")
    dec = shipped(golden, decoder).cuda().eval()
    dec.noise_generator = _fixed_noise(x["noise"])
    s = SPECS[decoder]
    hops = dict(phase=s["P"], voicing=s["P"], amp=s["hop"], wsel=s.get("wsel"))

    def args(lo, hi):
        sl = lambda v, hop: v[:, lo // hop: hi // hop]
        part = dict(x, harm=tuple(sl(v, s["hop"]) for v in x["harm"]),
                    noise_ctrl=tuple(sl(v, s["hop"]) for v in x["noise_ctrl"]),
                    **{k: sl(x[k], h) for k, h in hops.items() if k in x})
        return dict(_call_args(decoder, part), noise=AudioTensor(x["noise"][:, lo:hi]))

    return (lambda: HarmonicPlusNoiseStream(dec, B)), args, (lambda: dec(noise_generator_params=(), **_call_args(decoder, x)))


def _golf_case(B: int, T: int, decoder: str):
    """The same for golf-ss, golf-ff and golf-v1 over make_decoder's modules."""
    inp = make_inputs(B=B, T=T, device="cuda", with_noise_filter=True)
    if decoder == "golf-v1":
        dec = make_v1(inp["noise"]).cuda()
    else:
        dec = make_decoder(noise_filter=True, room_filter=True, injected_noise=inp["noise"],
                           framewise=decoder == "golf-ff").cuda()
    Stream = DecoderStream if decoder == "golf-ss" else FramewiseDecoderStream
    lpc_key = "harm_filter_params" if decoder == "golf-v1" else "end_filter_params"
    w_hop = inp["w_hop"]

    def args(lo, hi):
        fr = lambda k, hop: AudioTensor(inp[k][:, lo // hop: hi // hop], hop)
        return {"phase": AudioTensor(inp["phase"][:, lo:hi]), "harm_oscillator_params": (fr("wsel", w_hop),),
                "noise_filter_params": (fr("log_mag", 240),), lpc_key: (fr("gain", 240), fr("a", 240)),
                "noise": AudioTensor(inp["noise"][:, lo:hi])}

    full = lambda k, hop: AudioTensor(inp[k], hop)
    one_shot = lambda: dec(phase=AudioTensor(inp["phase"]), harm_oscillator_params=(full("wsel", w_hop),),
                           noise_generator_params=(), noise_filter_params=(full("log_mag", 240),),
                           **{lpc_key: (full("gain", 240), full("a", 240))})
    return (lambda: Stream(dec, batch_size=B)), args, one_shot


def run(B: int, push: int, T: int = 48000, reps: int = 3, decoder: str = "golf-ss") -> dict:
    make_stream, args, one_shot = (_hpn_case if decoder in HPN else _golf_case)(B, T, decoder)
    with torch.no_grad():
        times, total, n_out = _time_stream(make_stream, args, T, push, reps)
        one = []
        for _ in range(reps + 1):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            one_shot()
            e.record()
            e.synchronize()
            one.append(s.elapsed_time(e) * 1e3)
    dur = T / SR
    oneshot = min(one[1:])
    out = dict(B=B, push=push, pushes=len(times), samples_out=n_out, push_us=round(sum(times) / len(times), 1),
               push_us_max=round(max(times), 1), stream_total_us=round(total, 1), rtf=round(total * 1e-6 / dur, 5),
               oneshot_us=round(oneshot, 1), oneshot_rtf=round(oneshot * 1e-6 / dur, 5))
    return out if decoder == "golf-ss" else dict(decoder=decoder, **out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--decoder", choices=("golf-ss", "golf-ff", "golf-v1") + HPN, default="golf-ss")
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_stream.py needs a GPU"
    hop = 240 if opt.decoder in ("golf-ss", "golf-ff", "golf-v1", "ddsp") else 120
    for B in (1, 32):
        for push in sorted({hop, 240, 2400}):
            print(json.dumps(run(B, push, decoder=opt.decoder)), flush=True)
