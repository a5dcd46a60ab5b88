"""The frame-wise all-pole filter's ring kernels (csrc/lpc_ff.hip) on every template instance, route and tile edge: forward
and all three gradients through GF.lti_frames_ola, and the stream entry, against the float64 oracle on the cases of
tests/ff_ref.py (independent coefficient rows and gains per frame; which kernel each case takes is checked without a GPU in
tests/test_ff_ref_host.py).  Bars as in tests/test_gpu_lpc_ff_anyshape.py: forward <= 1e-4, each gradient <= 2e-4, relative
max-norm and L2.  Every comparison prints its distances and the worst of its group so far."""
import numpy as np
import pytest
import torch

import ff_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

WORST = {}          # group -> worst rel-max seen so far


def dev(x):
    return torch.as_tensor(np.array(x, dtype=np.float32)).cuda()   # (a copy: the shared cases are read-only)


def host(t):
    return t.detach().cpu().numpy()


def check(got, ref, what, bar, group):
    emax, el2 = rel_err(got, ref)
    WORST[group] = max(WORST.get(group, 0.0), emax)
    print(f"{what}: rel-max {emax:.3e} rel-l2 {el2:.3e}   [worst {group} so far {WORST[group]:.3e}]")
    assert np.isfinite(got).all(), what
    assert emax <= bar and el2 <= bar, (what, emax, el2)


def fwd_group(c):
    return c.fwd.split("<")[0]


def bwd_group(c):
    return "ring backward" if c.bwd.startswith("ring") else "any backward"


def leaves(arrays, grads=(True, True, True)):
    return tuple(dev(v).requires_grad_(g) for v, g in zip(arrays[:3], grads))


def run(c, arrays, grads=(True, True, True), x_in=None, gy_t=None, t=None):
    """Forward and backward through GF.lti_frames_ola; returns (y, g_ex, g_gain, g_a) as tensors.  ``t``: the leaves (made
    here otherwise); ``x_in``: the tensor handed in as the excitation when it is a view of the leaf; ``gy_t``: the cotangent
    tensor when it is not the contiguous one."""
    from golf_amd import functional as GF

    ex_t, gain_t, a_t = leaves(arrays, grads) if t is None else t
    y = GF.lti_frames_ola(ex_t if x_in is None else x_in, gain_t, a_t, dev(arrays[3]), c.hop)
    y.backward(dev(arrays[4]) if gy_t is None else gy_t)
    torch.cuda.synchronize()
    return y.detach(), ex_t.grad, gain_t.grad, a_t.grad


def check_all(c, got, want, what):
    for k, g in zip(R.OUTPUTS, got):
        assert g.shape == want[k].shape, (k, g.shape, want[k].shape)
        check(host(g), want[k], f"{what} {k}", R.BARS[k], fwd_group(c) if k == "y" else bwd_group(c))


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_one_shot_vs_oracle(c):
    check_all(c, run(c, R.inputs(c)), R.refs(c), R.case_id(c))


RAGGED = [(r, name) for r in R.RAGGED_ROWS for name in ("inside", "short", "long")]


@pytest.mark.parametrize("row,name", RAGGED, ids=[f"{R.case_id(r)}-{n}" for r, n in RAGGED])
def test_ragged_and_unused_frames(row, name):
    """The excitation ending inside the last frame, two frames short (nfr < F) and running on past (F-1)*hop + 1."""
    c = R.ragged(row)[name]
    Tx0, Tx, nfr, Ty = R.geometry(c)
    want = R.refs(c)
    y, g_ex, g_gain, g_a = run(c, R.inputs(c))
    assert y.shape == (c.B, Ty)
    check_all(c, (y, g_ex, g_gain, g_a), want, f"{R.case_id(c)} {name}")
    if name == "long":
        assert nfr == c.F and Tx0 > Tx and not g_ex[:, Tx:].any() and g_ex[:, :Tx].abs().sum() > 0
    else:
        assert nfr == c.F - (1 if name == "inside" else 2)
        assert not g_a[:, nfr:].any() and g_a[:, :nfr].abs().sum() > 0
        unused = (want["g_gain"] == 0).all(0)
        assert unused[-1] and np.array_equal(host(g_gain)[:, unused], want["g_gain"][:, unused])


@pytest.mark.parametrize("row", R.RAGGED_ROWS, ids=R.case_id)
def test_uncentred_module(row):
    """centred=False through LTVMinimumPhaseFilter: the first hop/2 samples dropped, the output reflect-padded."""
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import LTVMinimumPhaseFilter
    from oracle import golf_oracle as O

    c = R.ragged(row)["long"]
    ex, gain, a, win, _ = R.inputs(c)
    r_y, _ = O.lti_frames_ola_forward(ex, gain, a, c.hop, win, centred=False)
    gy = np.random.default_rng(1).normal(0, 1, r_y.shape).astype(np.float32)
    want = dict(zip(R.OUTPUTS, (r_y,) + tuple(O.lti_frames_ola_backward(gy, ex, gain, a, c.hop, win, centred=False))))
    m = LTVMinimumPhaseFilter(window="hanning", window_length=c.W, centred=False, lpc_order=c.M).cuda()
    t = leaves((ex, gain, a))
    y = m(AudioTensor(t[0]), AudioTensor(t[1], c.hop), AudioTensor(t[2], c.hop)).as_tensor()
    y.backward(dev(gy))
    torch.cuda.synchronize()
    check_all(c, (y, t[0].grad, t[1].grad, t[2].grad), want, f"{R.case_id(c)} uncentred")
    assert not t[0].grad[:, :c.hop // 2].any()


LAYOUT_ROWS = [R.first_case("block<6>")._replace(B=3, F=5), R.first_case("quad<32,30>")._replace(B=3),
               R.first_case("scalar<40,38>")]


@pytest.mark.parametrize("c", LAYOUT_ROWS, ids=R.case_id)
def test_layouts(c):
    """A column slice of a wider tensor as the excitation (rows with a stride of their own), a T-major excitation and a
    T-major cotangent (each copied to rows by the wrapper) give the bits of the contiguous call."""
    arrays = R.inputs(c)
    want = run(c, arrays)
    T = arrays[0].shape[1]
    # column slice
    wide = torch.zeros(c.B, T + 37, device="cuda")
    wide[:, 5:5 + T] = dev(arrays[0])
    wide.requires_grad_(True)
    view = wide[:, 5:5 + T]
    assert not view.is_contiguous()
    _, gain_t, a_t = leaves(arrays)
    y, g_wide, g_gain, g_a = run(c, arrays, t=(wide, gain_t, a_t), x_in=view)
    assert torch.equal(g_wide[:, 5:5 + T], want[1]) and not g_wide[:, :5].any() and not g_wide[:, 5 + T:].any()
    assert torch.equal(y, want[0]) and torch.equal(g_gain, want[2]) and torch.equal(g_a, want[3])
    # T-major excitation
    tm = dev(arrays[0]).t().contiguous().requires_grad_(True)
    assert tm.t().stride(1) != 1
    _, gain_t, a_t = leaves(arrays)
    y, g_tm, g_gain, g_a = run(c, arrays, t=(tm, gain_t, a_t), x_in=tm.t())
    assert torch.equal(g_tm.t(), want[1])
    assert torch.equal(y, want[0]) and torch.equal(g_gain, want[2]) and torch.equal(g_a, want[3])
    # T-major cotangent
    gy_t = dev(arrays[4]).t().contiguous().t()
    assert gy_t.stride(1) != 1
    for u, v in zip(run(c, arrays, gy_t=gy_t), want):
        assert torch.equal(u, v)


REPRO_ROWS = [R.first_case("quad<40,38>", "ring<40,38>")._replace(B=3, F=17), R.first_case("scalar<40,38>", "any")]


def test_partial_grads():
    """requires_grad on one input at a time gives the bits of the full backward (the ring chain; the wave-per-frame chain
    has this in tests/test_gpu_lpc_ff_anyshape.py)."""
    c = REPRO_ROWS[0]
    full = run(c, R.inputs(c))[1:]
    for only in range(3):
        grads = run(c, R.inputs(c), tuple(i == only for i in range(3)))[1:]
        for i in range(3):
            if i == only:
                assert torch.equal(grads[i], full[i])
            else:
                assert grads[i] is None


@pytest.mark.parametrize("c", REPRO_ROWS, ids=R.case_id)
def test_backward_is_reproducible(c):
    first, second = run(c, R.inputs(c)), run(c, R.inputs(c))
    for u, v in zip(first, second):
        assert torch.equal(u, v)


def outside(c, frames):
    """Mask of the output samples that none of ``frames`` reaches."""
    m = np.ones(R.geometry(c)[3], dtype=bool)
    for f in frames:
        m[R.span(c, f)] = False
    return torch.as_tensor(m).cuda()


@pytest.mark.parametrize("shape", R.TIER_SHAPES)
def test_conditioning_tier(shape):
    """The block recursion's two precision tiers side by side: twelve frames with planted rows -- wave 0 (frames 0..3) all
    kappa <= 16, wave 1 with frame 5 alone at kappa >= 256, wave 2 all at kappa >= 256 (kappa: ff_ref.kappa; GOLF_FF_KAPPA =
    64).  Forward within the bar on the whole and on every frame's own span, gradients within theirs; and with frame 5
    replaced by a low row the same bits wherever no frame of wave 1 reaches: the tier is decided per wave."""
    c, a, a_low, kappas = R.planted(shape)
    print(f"{shape}: kappa of the planted frames", " ".join(f"{k:.1f}" for k in kappas[:-1]), f"; swapped in: {kappas[-1]:.1f}")
    outs = []
    for rows, tag in ((a, "planted"), (a_low, "wave 1 low")):
        got, want = run(c, R.inputs(c, rows)), R.refs(c, rows)
        check_all(c, got, want, f"tier {shape} {tag}")
        for f, (emax, el2) in enumerate(R.span_distances(c, host(got[0]), want["y"])):
            print(f"tier {shape} {tag} frame {f} (kappa {R.kappa(rows[0, f], shape[0]):.1f}): rel-max {emax:.3e} rel-l2 {el2:.3e}")
            assert emax <= R.TOL_Y and el2 <= R.TOL_Y, (tag, f, emax, el2)
        outs.append(got)
    (y, g_ex, g_gain, g_a), (y2, g_ex2, g_gain2, g_a2) = outs
    away = outside(c, range(4, 8))
    assert 0 < int(away.sum()) < away.numel()
    assert torch.equal(y[:, away], y2[:, away])
    print(f"tier {shape}: samples of wave 1 that frame {R.SWAPPED} does not reach and that changed bits:",
          int((y != y2)[:, ~away & outside(c, [R.SWAPPED])].sum()))
    # the adjoint and g_a run per frame: only frame 5's row, and what its span reaches, may move with it
    off5 = outside(c, [R.SWAPPED])
    assert torch.equal(g_ex[:, :-1][:, off5], g_ex2[:, :-1][:, off5]) and torch.equal(g_ex[:, -1], g_ex2[:, -1])
    keep = [f for f in range(c.F) if not 4 <= f < 8]
    assert torch.equal(g_a[:, keep], g_a2[:, keep]) and not torch.equal(g_a[:, R.SWAPPED], g_a2[:, R.SWAPPED])


def stream(c, arrays, cuts):
    from test_gpu_stream_ff import _stream_filter

    ex, gain, a, win = (dev(v) for v in arrays[:4])
    return _stream_filter(ex, gain, a, win, c.hop, cuts)


@pytest.mark.parametrize("c", R.STREAM_CASES, ids=lambda c: f"{R.case_id(c)}-stream-{c.stream}")
def test_stream_kernels(c):
    """Each of the eight stream kernels: against the oracle (<= 1e-4) and the one-shot entry (<= 2e-4), the contract of
    tests/test_gpu_stream_ff.py; three random splits, zero-length calls included, give the bits of the single call."""
    from golf_amd import functional as GF
    from test_gpu_stream_ff import _random_cuts

    arrays = R.inputs(c)
    nfr = R.geometry(c)[2]
    whole = stream(c, arrays, [])
    check(host(whole), R.refs(c)["y"], f"stream {c.stream} {R.case_id(c)} vs oracle", R.TOL_Y, "stream")
    with torch.no_grad():
        one = GF.lti_frames_ola(*(dev(v) for v in arrays[:4]), c.hop)
    assert one.shape == whole.shape
    emax, el2 = rel_err(host(whole), host(one))
    print(f"stream {c.stream} vs one-shot: rel-max {emax:.3e} rel-l2 {el2:.3e}")
    assert emax <= 2e-4, emax
    rng = np.random.default_rng([c.M, c.hop, c.W])
    for _ in range(3):
        assert torch.equal(stream(c, arrays, _random_cuts(rng, nfr)), whole)


@pytest.mark.parametrize("shape", R.TIER_SHAPES)
def test_stream_tier_is_per_frame(shape):
    """The planted utterance of the tier test through the stream entry: within the bar, and replacing the one high frame
    of wave 1 by a low row changes no bit of any sample outside that frame's own span -- stricter than the one-shot's
    per-wave tier, and what the stream's split invariance rests on (a frame's wave mates depend on the split)."""
    from test_gpu_stream_ff import _random_cuts

    c, a, a_low, _ = R.planted(shape)
    assert c.stream == f"block<{shape[0]}>"
    y = stream(c, R.inputs(c, a), [])
    y2 = stream(c, R.inputs(c, a_low), [])
    check(host(y), R.refs(c, a)["y"], f"stream tier {shape} planted", R.TOL_Y, "stream")
    check(host(y2), R.refs(c, a_low)["y"], f"stream tier {shape} wave 1 low", R.TOL_Y, "stream")
    away = outside(c, [R.SWAPPED])
    assert 0 < int(away.sum()) < away.numel()
    assert torch.equal(y[:, away], y2[:, away]) and not torch.equal(y[:, ~away], y2[:, ~away])
    rng = np.random.default_rng(5)
    for _ in range(3):    # frame 5 in a wave with other mates each time
        assert torch.equal(stream(c, R.inputs(c, a), _random_cuts(rng, c.F)), y)


def test_zz_worst_values_per_group():
    """Not a check: the worst rel-max of every group, for the record (-s shows it)."""
    for g, v in sorted(WORST.items()):
        print(f"worst rel-max, {g}: {v:.3e}")
