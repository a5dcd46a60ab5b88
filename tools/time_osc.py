"""dev: time the glottal oscillator forward over batch sizes (GOLF_HIP_LIBRARY selects a variant build).
usage: python tools/time_osc.py [B ...]     (default: 32 512)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def one(B, iters=20):
    import torch
    from golf_amd import functional as GF
    from golf_amd.synth import DownsampledIndexedGlottalFlowTable
    from golf_amd.synthetic import make_inputs

    inp = make_inputs(B=min(B, 64), device="cuda")
    rep = (B + 63) // 64
    phase = inp["phase"].repeat(rep, 1)[:B].contiguous()
    wsel = inp["wsel"].repeat(rep, 1)[:B].contiguous()
    noise = inp["noise"].repeat(rep, 1)[:B].contiguous()
    osc = DownsampledIndexedGlottalFlowTable(hop_rate=10, in_channels=64, oversampling=4, equal_energy=True, lf_v2=True,
                                             points=2048).cuda()
    f = lambda: GF.glottal_osc(phase, wsel, osc.table, osc.decimater.taps, 1, inp["w_hop"], 4, True, add=noise)
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    print(f"B={B}: {us:9.1f} us/call  {us / B:7.3f} us/utterance", flush=True)


if __name__ == "__main__":
    for B in [int(v) for v in sys.argv[1:]] or [32, 512]:
        one(B)
