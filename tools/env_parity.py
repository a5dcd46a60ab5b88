"""Parity of the spectral-envelope analysis kernel (csrc/spec_envelope.hip) on every case of tests/env_ref.py, dev tool: the
largest errors of the GPU against the float64 restatement, and of the restatement's fp32 stand-in against it, in the units of
tests/test_gpu_env.py: magnitudes exp(log_env) in units of the frame's largest reference magnitude (bar 1e-4) and ceps in
nepers (bar: 4 x the stand-in's largest, rounded up to one digit).  Writes profiles/env_parity.txt, or the file given as the
first argument."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import env_ref as R
from golf_amd import functional as GF

lines = []
worst = np.zeros((2, 2))
for name, (x, f0, kw) in R.cases().items():
    ref = R.reference(name)
    low = R.analyse(x, f0, fp32=True, **kw)
    kw = dict(dict(n_ceps=kw["n_fft"] // 2 + 1), **kw)
    out = GF.spectral_envelope(torch.tensor(x).cuda(), torch.tensor(f0).cuda(), kw.pop("sample_rate"), kw.pop("hop"), **kw)
    got = dict(log_env=out[0].cpu().numpy().astype(np.float64), ceps=out[1].cpu().numpy().astype(np.float64))
    e = np.array([R.errors(got, ref), R.errors(low, ref)])
    worst = np.maximum(worst, e)
    lines.append(f"{name:12s} {ref['voiced'].size:3d} frames   gpu: magnitudes {e[0, 0]:.2e} ceps {e[0, 1]:.2e} Np"
                 f"   fp32 stand-in: magnitudes {e[1, 0]:.2e} ceps {e[1, 1]:.2e} Np")
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "env_parity.txt")
with open(out, "w") as f:
    f.write(f"{torch.cuda.get_device_name(0)}: spectral_envelope against tests/env_ref.py (float64) on the cases of its cases(); "
            "largest error per case: magnitudes exp(log_env) in units of the frame's largest reference magnitude (the bar of "
            "tests/test_gpu_env.py is 1e-4), ceps in nepers (its bar is 4 x the stand-in's largest, rounded up to one digit)\n")
    f.write("\n".join(lines) + "\n")
    f.write(f"largest                   gpu: magnitudes {worst[0, 0]:.2e} ceps {worst[0, 1]:.2e} Np"
            f"   fp32 stand-in: magnitudes {worst[1, 0]:.2e} ceps {worst[1, 1]:.2e} Np\n")
    f.write(f"ceps bar: 4 x {worst[1, 1]:.2e} = {4 * worst[1, 1]:.2e} Np\n")
print(open(out).read())
