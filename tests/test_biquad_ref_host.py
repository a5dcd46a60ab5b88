"""The yardsticks of the cascaded-biquad GPU tests, checked on the CPU at every shape those tests use
(tests/biquad_ref.py): the float64 oracle's forward and closed-form backward against a plain float64 torch cascade and its
autograd, and the sequential float32 cascade's distance from the oracle on make_case's inputs -- the condition the GPU
tests' bound, 1e-4 + 3 x that distance, rests on."""
import numpy as np
import pytest

import biquad_ref as R
from conftest import rel_err


@pytest.mark.parametrize("cid", list(R.CASES))
def test_oracle_agrees_with_torch_autograd(cid):
    from oracle import golf_oracle as O

    c = R.case(cid)
    ex, gain, bq, win, pad, hop, fg = (c[k] for k in ("ex", "gain", "bq", "win", "pad", "hop", "frame_gain"))
    ref = O.biquad_frames_ola_forward(ex, gain, bq, hop, win, pad=pad, frame_gain=fg)
    gy = R.make_gy(ref, c["seed"])
    refs = (ref,) + tuple(O.biquad_frames_ola_backward(gy, ex, gain, bq, hop, win, pad=pad, frame_gain=fg))
    outs = R.torch_cascade_f64(ex, gain, bq, hop, win, pad=pad, frame_gain=fg, gy=gy)
    assert ref.shape == (c["B"], c["Ty"])
    for name, got, want in zip(("y", "g_ex", "g_gain", "g_biquads"), refs, outs):
        emax, el2 = rel_err(got, want)
        print(f"{cid} {name}: oracle vs float64 torch rel-max {emax:.3e} rel-l2 {el2:.3e}")
        assert emax <= 1e-10 and el2 <= 1e-10, (cid, name, emax, el2)
    # the parts no frame reaches are zero in both
    nfr, used = c["nfr"], c["used"]
    for g_ex, g_gain, g_bq in (refs[1:], outs[1:]):
        assert np.all(g_bq[:, nfr:] == 0) and np.all(g_ex[:, used:] == 0)
        if fg:
            assert np.all(g_gain[:, nfr:] == 0)


@pytest.mark.parametrize("cid", list(R.CASES))
def test_sequential_fp32_error(cid):
    from oracle import golf_oracle as O

    c = R.case(cid)
    ex, gain, bq, win, pad, hop, fg = (c[k] for k in ("ex", "gain", "bq", "win", "pad", "hop", "frame_gain"))
    ref = O.biquad_frames_ola_forward(ex, gain, bq, hop, win, pad=pad, frame_gain=fg)
    emax, el2 = rel_err(R.cascade_f32(ex, gain, bq, hop, win, pad=pad, frame_gain=fg), ref)
    print(f"{cid}: sequential fp32 cascade rel-max {emax:.3e} rel-l2 {el2:.3e}")
    # default inputs: 1e-4, so the GPU bound never exceeds 4e-4; the harsh inputs: the cap of 1e-3 (bound <= 3.1e-3)
    assert emax <= (1e-3 if cid in R.HARSH_SHAPES else 1e-4), (cid, emax)


def test_the_shapes_cover_what_they_are_named_for():
    """The boundaries the shape tables claim, computed from the kernels' own launch arithmetic (csrc/lpc_ff.hip)."""
    fg = [R.case(cid) for cid in R.FRAME_GAIN_SHAPES]
    allc = [R.case(cid) for cid in R.CASES]
    blocks = {(c["W"] + c["K"] - 1 + 3) // 4 % 2 for c in allc}
    assert blocks == {0, 1}
    assert {c["nfr"] % 4 for c in allc} == {0, 1, 2, 3} and any(c["nfr"] == 1 for c in allc)
    assert {1, 2, 16} <= {c["K"] for c in allc}
    xs = sorted((3 * c["hop"] + c["W"] + 40 + 3) // 4 * 4 for c in allc)
    assert xs[0] < 512 and any(512 < v < 1024 for v in xs) and xs[-1] > 1536
    ws = {c["W"] for c in allc}
    assert any(w < 64 for w in ws) and 64 in ws and any(w > 64 and w % 64 for w in ws) and any(w % 4 for w in ws)
    assert any(c["F"] > c["nfr"] for c in fg) and any(c["Tx"] > c["used"] for c in fg)
    for c in allc:   # every shape is inside both LDS limits
        assert 4 * (3 * c["hop"] + 5 * c["W"] + 168 + 3) <= 60 * 1024 and (c["K"] + 2) * (c["W"] + 4) * 4 <= 65536


@pytest.mark.parametrize("hop,F,T", [(8, 4, 25), (8, 4, 19), (8, 4, 1), (4, 2, 5), (4, 2, 3), (1, 5, 5), (16, 1, 1)])
def test_upsample_adjoint_is_the_oracles(hop, F, T):
    """golf_amd.functional.upsample_adjoint (plain torch; it folds the interpolated-gain gradient of the cascade onto the
    gain frames) against the oracle's scatter-add, in float64, for a full, a short and a one-sample input."""
    import torch
    from golf_amd.functional import upsample_adjoint
    from oracle import golf_oracle as O

    v = np.random.default_rng(hop + F + T).normal(0, 1, (3, T))
    got = upsample_adjoint(torch.from_numpy(v), hop, F).numpy()
    emax, _ = rel_err(got, O._upsample_adjoint(v, hop, F))
    assert got.shape == (3, F) and emax <= 1e-14, emax
