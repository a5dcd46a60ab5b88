"""Parity of the harmonic-plus-noise analysis kernel (csrc/harm_analysis.hip) on every case of tests/hna_ref.py, dev tool:
the largest amplitude, magnitude and phase errors of the GPU against the float64 oracle, and of the oracle's fp32 stand-in
against it, in the units of tests/test_gpu_hna.py (the frame's scale, max |x| over its window; its bar is 1e-4).  Writes
profiles/hna_parity.txt, or the file given as the first argument."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import hna_ref as R
from golf_amd import functional as GF

lines = []
worst = np.zeros((2, 3))
for name, (x, f0, kw) in R.cases().items():
    ref = R.reference(name)
    low = R.analyse(x, f0, fp32=True, **kw)
    kw = dict(kw)
    out = GF.harmonic_analysis(torch.tensor(x).cuda(), torch.tensor(f0).cuda(), kw.pop("sample_rate"), kw.pop("hop"), kw.pop("K"),
                               n_mag=kw.pop("n_mag") or None, return_phases=True, **kw)
    arr = [t.cpu().numpy().astype(np.float64) for t in out]
    got = dict(amp=arr[0], phase=arr[1], log_mag=arr[2] if len(arr) == 3 else None)
    e = np.array([R.errors(got, ref), R.errors(low, ref)])
    worst = np.maximum(worst, e)
    lines.append(f"{name:16s} {ref['scale'].size:4d} frames   gpu: amp {e[0, 0]:.2e} mag {e[0, 1]:.2e} phase {e[0, 2]:.2e}"
                 f"   fp32 stand-in: amp {e[1, 0]:.2e} mag {e[1, 1]:.2e} phase {e[1, 2]:.2e}")
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hna_parity.txt")
with open(out, "w") as f:
    f.write(f"{torch.cuda.get_device_name(0)}: harmonic_analysis against tests/hna_ref.py (float64) on the cases of its cases(); "
            "largest error per case in units of the frame's scale (max |x| over its window); phase error times amp / scale; "
            "the bar of tests/test_gpu_hna.py is 1e-4\n")
    f.write("\n".join(lines) + "\n")
    f.write(f"largest            gpu: amp {worst[0, 0]:.2e} mag {worst[0, 1]:.2e} phase {worst[0, 2]:.2e}"
            f"   fp32 stand-in: amp {worst[1, 0]:.2e} mag {worst[1, 1]:.2e} phase {worst[1, 2]:.2e}\n")
print(open(out).read())
