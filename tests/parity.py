"""Shared helpers of the GPU parity tests (TEST INFRASTRUCTURE): float64 / fp32 runs of a PyTorch restatement on the CPU,
the per-frame error check of the control transforms, and a per-family record of the worst figures seen.

Per-frame check.  conftest.rel_err divides by the largest entry of the whole tensor, so one wrong frame can hide behind a
louder one -- which is how a per-lane or tail-block error of a frame-per-thread kernel would look.  So every frame (row of
the (N, M) view) is also judged on its own:

    err_f   = max_i |x[f,i] - ref[f,i]| / max_i |ref[f,i]|
    allow_f = max(tol, 4 * r_f)

with tol the global bound of the case and r_f the same quantity for the restatement run in fp32 on the CPU: the
reference's own rounding, never the kernel's.  The factor 4 is the project's 2-3x the reference's own fp32 result plus room
for the kernel ordering its sums differently.  The share of frames with 4 * r_f > tol is capped by the caller, so that the
loosened allowance cannot quietly exempt the frames."""
import numpy as np
import torch

from conftest import rel_err


def dev(x, grad=False):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32).cuda().requires_grad_(grad)


def torch_restatement(fn, x, gy, dtype):
    """fn on the CPU in ``dtype``: (values, gradient w.r.t. x of sum(values * gy)) as float64 arrays."""
    xin = x.detach().cpu().to(dtype).requires_grad_(True)
    out = fn(xin)
    (out * gy.detach().cpu().to(dtype)).sum().backward()
    return out.detach().double().numpy(), xin.grad.double().numpy()


def frame_err(x, ref):
    """err_f of every frame: x, ref (..., M) -> (N,)"""
    x = np.asarray(x, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    x, ref = x.reshape(-1, x.shape[-1]), ref.reshape(-1, ref.shape[-1])
    return np.abs(x - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-300)


def frame_check(got, ref64, ref32, tol):
    """(worst err_f / allow_f, the frame it occurs at with its err_f and r_f, share of frames on the loosened allowance
    4 * r_f > tol)"""
    e, r = frame_err(got, ref64), frame_err(ref32, ref64)
    ratio = e / np.maximum(tol, 4.0 * r)
    worst = int(np.argmax(ratio))
    return float(ratio[worst]), (worst, float(e[worst]), float(r[worst])), float(np.mean(4.0 * r > tol))


class Worst:
    """Running worst figures of one family of tests; every note() prints the figures of the case and the family's worst so
    far, so the last line a family prints is its overall worst."""

    def __init__(self, family):
        self.family = family
        self.glob = self.ratio = self.share = 0.0

    def note(self, what, glob, ratio=None, share=None):
        self.glob = max(self.glob, glob)
        line = f"{what}: global {glob:.2e}"
        tail = f" | {self.family} worst so far: global {self.glob:.2e}"
        if ratio is not None:
            self.ratio, self.share = max(self.ratio, ratio), max(self.share, share)
            line += f", err_f/allow_f {ratio:.3f}, loosened frames {100 * share:.1f}%"
            tail += f", err_f/allow_f {self.ratio:.3f}, loosened frames {100 * self.share:.1f}%"
        print(line + tail)


def check_global(worst, what, got, ref, tol):
    """Both conftest.rel_err norms of ``got`` against ``ref`` within ``tol``, recorded in ``worst``."""
    emax, el2 = rel_err(np.asarray(got), np.asarray(ref))
    worst.note(what, max(emax, el2))
    assert emax < tol and el2 < tol, (what, emax, el2, tol)


def check_frames(worst, what, got, ref64, ref32, tol, cap):
    """Global bound, per-frame bound and the cap on loosened frames of one (..., M) result."""
    emax, el2 = rel_err(np.asarray(got), ref64)
    ratio, frame, share = frame_check(got, ref64, ref32, tol)
    worst.note(what, max(emax, el2), ratio, share)
    assert share <= cap, (what, "the fp32 restatement alone is beyond the bound on too many frames", share, cap)
    assert emax < tol and el2 < tol, (what, emax, el2, tol)
    assert ratio <= 1.0, (what, "(frame, err_f, r_f)", frame, "err_f / allow_f", ratio)
