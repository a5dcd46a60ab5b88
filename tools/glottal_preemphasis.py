"""What the inverse filter is worth to the glottal-source analysis, dev tool, no GPU: tests/glottal_ref.py (float64) on pulses
of the package's table at a constant table position, through a fixed 5-formant all-pole filter, with the residual taken by
(a) the true inverse filter, (b) a whole-signal order-22 LPC (autocorrelation method) of the audio itself, (c) the same LPC
computed on 0.97-pre-emphasised audio and applied to the audio.  Prints the largest / rms error of w in table steps on
interior frames; the figures are quoted in INTEGRATION.md 2h."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import glottal_ref as R

FORMANTS = ((700.0, 90.0), (1220.0, 110.0), (2600.0, 160.0), (3500.0, 200.0), (4500.0, 250.0))   # Hz, bandwidth


def allpole():
    a = np.ones(1)
    for fc, bw in FORMANTS:
        r = np.exp(-np.pi * bw / R.SR)
        a = np.convolve(a, [1.0, -2 * r * np.cos(2 * np.pi * fc / R.SR), r * r])
    return a


def synth(e, a):
    y = np.zeros(len(e))
    for t in range(len(e)):
        y[t] = e[t] - sum(a[i] * y[t - i] for i in range(1, min(len(a), t + 1)))
    return y


def lpc(x, order):
    r = np.array([np.dot(x[:len(x) - i], x[i:]) for i in range(order + 1)])
    T = np.array([[r[abs(i - j)] for j in range(order)] for i in range(order)])
    return np.concatenate([[1.0], np.linalg.solve(T + 1e-9 * r[0] * np.eye(order), -r[1:])])


for w0 in (0.3, 0.7):
    f0, _ = R.planted_tracks()
    case = R.build_case(R.golf_table(), 64, 256, list(f0), [np.full(f0.shape[1], w0)], 31, noise=0.01)
    e = case["x"][0].astype(np.float64)
    a_true = allpole()
    y = synth(e, a_true)
    pre = np.concatenate([[y[0]], y[1:] - 0.97 * y[:-1]])
    for label, a in (("the true inverse filter", a_true), ("order-22 LPC of the audio", lpc(y, 22)),
                     ("order-22 LPC of the 0.97-pre-emphasised audio", lpc(pre, 22))):
        res = np.convolve(y, a)[:len(y)]
        amp, ph = R.harmonics(case, res[None].astype(np.float32))
        w_max, w_rms, _ = R.planted_errors(case, R.run(case, amp, ph))
        print(f"w = {w0}: {label:48s} w max {w_max:.2f} rms {w_rms:.2f} steps")
