"""Parity of the glottal-source match kernel (csrc/glottal_match.hip) on every case of tests/glottal_ref.py, dev tool: the
largest errors of the GPU against the float64 restatement on the kernel's own harmonics, and of the restatement's fp32
stand-in against it, in the units of tests/test_gpu_glottal.py: rho, theta in cycles, w in table steps (bars: 4 x the
stand-in's largest).  Writes the section "kernel" of profiles/glottal_parity.txt, or of the file given as the first argument,
and keeps the section before it.  ``--host`` (no GPU) writes that first section instead: what the float64 restatement itself
is worth on the planted cases of tests/test_glottal_host.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import glottal_ref as R

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out = args[0] if args else os.path.join(ROOT, "profiles", "glottal_parity.txt")
head = "== kernel =="
if "--host" in sys.argv:
    def measured(case, x=None):
        amp, ph = R.harmonics(case, x)
        return R.run(case, amp, ph)

    rows = []
    for label, case in (("random-walk w, 1 % noise, 64 harmonics, 256 shifts", R.planted_case()),
                        ("constant w = 0.3", R.planted_case("const")), ("16 harmonics", R.planted_case(H=16)),
                        ("64 shifts", R.planted_case(n_phi=64)), ("10 % noise, 32 harmonics, 128 shifts", R.planted_case("walk", 0.1, 32, 128)),
                        ("the oscillator's rendition (float64 oracle, oversampling 4), no noise", R.round_trip_case())):
        res = measured(case)
        rows.append("%-72s w max %.4f rms %.4f steps   theta %.3e cycles   rho >= %.4f" % (
            (label,) + R.planted_errors(case, res) + (R.interior(res["rho"]).min(),)))
    case = R.planted_case()
    noise = measured(case, np.random.default_rng(5).normal(0, 1, case["x"].shape).astype(np.float32))["rho"]
    kept = open(out).read().split(head)[1] if os.path.exists(out) and head in open(out).read() else None
    with open(out, "w") as f:
        f.write("tests/glottal_ref.py (float64) on planted table positions: the package's 100 x 1000 table, one row of 40 frames, "
                "the glide 110-180 Hz with vibrato, interior frames (all but two at either end); band-limited pulses of the "
                "table's spectrum unless said otherwise\n")
        f.write("\n".join(rows) + "\n")
        f.write("white noise through the same analysis: rho <= %.4f (mean %.4f); the bar between noise and voiced frames is %.2f\n"
                % (noise.max(), noise.mean(), R.RHO_BAR))
        if kept is not None:
            f.write(head + kept)
    print(open(out).read())
    sys.exit(0)

from golf_amd import functional as GF

lines = []
worst = np.zeros((2, 3))
for name, c in R.cases().items():
    f0 = torch.tensor(c["f0"]).cuda()
    amp, ph = GF.harmonic_analysis(torch.tensor(c["x"]).cuda(), f0, c["sample_rate"], c["hop"], c["H"], return_phases=True)
    res = GF.glottal_match(amp, ph, f0, GF.glottal_plan(torch.tensor(c["table"]).cuda(), c["H"]), c["sample_rate"], c["n_phi"])
    got = {k: t.cpu().numpy().astype(np.float64) for k, t in zip(("w", "theta", "rho"), res)}
    a, p = amp.cpu().numpy(), ph.cpu().numpy()
    ref, low = R.run(c, a, p), R.run(c, a, p, fp32=True)
    K = c["table"].shape[0]
    e = np.array([R.errors(got, ref, K)[:3], R.errors(low, ref, K)[:3]])
    worst = np.maximum(worst, e)
    lines.append(f"{name:10s} {ref['w'].size:3d} frames, {100 * R.errors(got, ref, K)[3]:.1f} % left out of w   "
                 f"gpu: rho {e[0, 0]:.2e} theta {e[0, 1]:.2e} w {e[0, 2]:.2e}   "
                 f"fp32 stand-in: rho {e[1, 0]:.2e} theta {e[1, 1]:.2e} w {e[1, 2]:.2e}")
kept = open(out).read().split(head)[0] if os.path.exists(out) else ""
with open(out, "w") as f:
    f.write(kept)
    f.write(f"{head}\n{torch.cuda.get_device_name(0)}: glottal_match against tests/glottal_ref.py (float64) on the kernel's own "
            "harmonics, the cases of its cases(); largest error per case: rho, theta in cycles, w in table steps (the bars of "
            "tests/test_gpu_glottal.py: 4 x the stand-in's largest over the cases)\n")
    f.write("\n".join(lines) + "\n")
    f.write(f"largest    gpu: rho {worst[0, 0]:.2e} theta {worst[0, 1]:.2e} w {worst[0, 2]:.2e}   "
            f"fp32 stand-in: rho {worst[1, 0]:.2e} theta {worst[1, 1]:.2e} w {worst[1, 2]:.2e}\n")
print(open(out).read())
