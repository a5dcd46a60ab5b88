"""Device time per DecoderStream.push and the real-time factor of streaming golf-ss synthesis, beside the one-shot decoder on
the same audio.  Needs a GPU; run under a time limit, e.g.  timeout -k 10 600 python tools/time_stream.py

For B in {1, 32} and pushes of 240 and 2400 samples (every track sliced to the same stretch of time), 2 s utterances:
  push_us     mean device time of one push (CUDA events around the push, synchronised per push: the host side is included)
  rtf         device time of the whole stream / audio duration (24 kHz)
  oneshot_us  device time of one decoder(...) call on the whole utterance, and its rtf
One JSON line per configuration."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from golf_amd.audiotensor import AudioTensor  # noqa: E402
from golf_amd.stream import DecoderStream  # noqa: E402
from golf_amd.synthetic import make_decoder, make_inputs  # noqa: E402

SR = 24000


def run(B: int, push: int, T: int = 48000, reps: int = 3) -> dict:
    inp = make_inputs(B=B, T=T, device="cuda", with_noise_filter=True)
    dec = make_decoder(noise_filter=True, room_filter=True, injected_noise=inp["noise"]).cuda()
    w_hop = inp["w_hop"]

    def args(lo, hi):
        fr = lambda k, hop: AudioTensor(inp[k][:, lo // hop: hi // hop], hop)
        return dict(phase=AudioTensor(inp["phase"][:, lo:hi]), harm_oscillator_params=(fr("wsel", w_hop),),
                    noise_filter_params=(fr("log_mag", 240),), end_filter_params=(fr("gain", 240), fr("a", 240)),
                    noise=AudioTensor(inp["noise"][:, lo:hi]))

    times, total, n_out = [], 0.0, 0
    with torch.no_grad():
        for _ in range(reps):
            st = DecoderStream(dec, batch_size=B)
            times, total, n_out = [], 0.0, 0
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
        one = []
        for _ in range(reps + 1):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            dec(phase=AudioTensor(inp["phase"]), harm_oscillator_params=(AudioTensor(inp["wsel"], w_hop),),
                noise_generator_params=(), noise_filter_params=(AudioTensor(inp["log_mag"], 240),),
                end_filter_params=(AudioTensor(inp["gain"], 240), AudioTensor(inp["a"], 240)))
            e.record()
            e.synchronize()
            one.append(s.elapsed_time(e) * 1e3)
    dur = T / SR
    oneshot = min(one[1:])
    return dict(B=B, push=push, pushes=len(times), samples_out=n_out, push_us=round(sum(times) / len(times), 1),
                push_us_max=round(max(times), 1), stream_total_us=round(total, 1), rtf=round(total * 1e-6 / dur, 5),
                oneshot_us=round(oneshot, 1), oneshot_rtf=round(oneshot * 1e-6 / dur, 5))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "tools/time_stream.py needs a GPU"
    for B in (1, 32):
        for push in (240, 2400):
            print(json.dumps(run(B, push)), flush=True)
