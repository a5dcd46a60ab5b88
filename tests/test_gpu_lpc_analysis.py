"""GPU parity of the frame-wise LPC analysis (golf_lpc_analysis_{fwd,bwd}_f32, functional.lpc_analysis, lpc.LPCAnalysis)
against the float64 restatement of its definition (tests/lpc_analysis_ref.py, pinned to oracle/make_lpc_tracks.py by
tests/test_lpc_analysis_host.py) on the same fp32 inputs.

Audio: seeded noise through the all-pole filters of tests/golden/g25 (speech tracks; reflection coefficients up to 0.998), a
stretch of exact zeros in one row; pure seeded noise at the small shapes.

Bars: the project's parity bar, 1e-4 (TOL of the LPC suites), per frame with no frame left out -- a: rel-max over the frame's
coefficients (1e-6 absolute where the reference is exactly 0: silent frames), rc: absolute, gain: relative; g_x: rel-max
and rel-L2 over the batch.  What clears the bar and what does not (CPU probe on this audio, against all-float64): the
windowed frame rounded to fp32 with fp64 lags and recursion <= 2.5e-6; an fp32 recursion on exact lags 7e-4 .. 4e-3; fp32
lags 1e-3 .. 9e-2.  The float64 gradient itself moves by 2.3e-6 rel-max under a 6e-8 relative perturbation of x.

The widest windows (W > 2048, two-wave workgroups) on the same CPU probe, the windowed frame rounded to fp32 and everything
after it in fp64: forward W2049 a 4.3e-7, rc 1.7e-7, gain 1.5e-7; W4096_M64 a 1.1e-6, rc 2.6e-7, gain 1.6e-8.  The float64
gradient moves under a 6e-8 relative perturbation of x by 2.2e-6 (W2049), 1.1e-5 (W4096_M64: a ninth of the bar) and 2.2e-6
(W4095_from0).  Measured on an MI355X (forward a / rc / gain; the largest g_x rel-max over the four cotangent sets): W2049
7.8e-7 / 2.1e-7 / 5.2e-8, g_x 5.6e-6; W4096_M64 1.1e-6 / 2.5e-7 / 7.1e-8, g_x 6.0e-6; W4095_from0 3.8e-8 / 2.4e-8 / 4.2e-8,
g_x 1.5e-6; M1 3.0e-6 / 2.7e-8 / 7.8e-8, g_x 4.9e-8; M7 1.4e-7 / 3.1e-8 / 6.0e-8, g_x 9.7e-8; M63 2.3e-7 / 2.5e-8 / 5.5e-8,
g_x 2.3e-7."""
import functools

import numpy as np
import pytest
import torch

import lpc_analysis_ref as R
from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4

# name -> (B, T, W, hop, M, centred, n_frames, audio)
CASES = {
    "recipe": (2, 4801, 960, 240, 22, True, None, "speech"),
    "edges": (3, 1000, 960, 240, 22, True, None, "speech"),
    "order64": (2, 4801, 960, 240, 64, True, None, "speech"),
    "odd50": (5, 777, 50, 7, 13, True, None, "noise"),
    "odd51": (5, 777, 51, 7, 13, True, None, "noise"),
    "hop>W": (1, 300, 128, 200, 8, True, None, "noise"),
    "W>T": (2, 100, 256, 64, 4, True, None, "noise"),
    "from0": (2, 4801, 960, 240, 22, False, None, "speech"),
    "more_frames": (5, 777, 50, 7, 13, True, 130, "noise"),
    "strided": (3, 1000, 256, 64, 16, True, None, "noise-strided"),
    # W > 2048: two-wave workgroups (another LDS slice layout, another workgroup-to-frame mapping).  T = 4800, not 4801: the
    # silent-stretch assertions hang on T == 4801 and presume windows of 960
    "W2049": (3, 4800, 2049, 600, 22, True, None, "speech"),         # the first width on two waves, odd
    "W4096_M64": (3, 4800, 4096, 1200, 64, True, None, "speech"),    # both limits
    "W4095_from0": (3, 4800, 4095, 1200, 9, False, None, "speech"),  # F = 1: G = 3 leaves a two-wave workgroup half idle
    # the orders at the ends of the lag passes and of the recursion's lanes
    "M1": (5, 777, 50, 7, 1, True, None, "noise"),                   # the smallest order
    "M7": (5, 777, 50, 7, 7, True, None, "noise"),                   # the last lag of the first LA_LAGS pass
    "M63": (5, 777, 128, 7, 63, True, None, "noise"),                # one lane idle in the recursion
}
SILENT = slice(1500, 3500)   # row 1 of the speech cases with T = 4801
COTANGENTS = ("all", "gain", "a", "rc")


def _golden(name):
    import os

    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs (fp32), cotangents and the float64 reference of one case: computed once, shared by the tests, never changed."""
    B, T, W, hop, M, centred, n_frames, audio = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if audio == "speech":
        x = R.speech_like(_golden, (0, 9, 4)[:B], T, seed=0)
        if T == 4801:
            x[1, SILENT] = 0.0
    else:
        x = rng.normal(0, 1, (B, T))
    x = x.astype(np.float32)
    window = torch.hann_window(W)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    out = R.analysis(xt, window, hop, M, centred=centred, n_frames=n_frames)
    cot = tuple(rng.normal(0, 1, tuple(o.shape)).astype(np.float32) for o in out)
    g_x = {}
    for which in COTANGENTS:
        loss = sum((o * torch.tensor(g).double()).sum()
                   for o, g, nm in zip(out, cot, ("gain", "a", "rc")) if which in ("all", nm))
        g_x[which] = torch.autograd.grad(loss, xt, retain_graph=True)[0].numpy()
    ref = tuple(o.detach().numpy() for o in out)
    for arr in (x, *cot, *ref, *g_x.values()):
        arr.setflags(write=False)
    return x, window, cot, ref, g_x


def device_x(name, grad=False):
    x = case(name)[0]
    if CASES[name][-1] == "noise-strided":   # rows of a wider buffer: unit inner stride, row stride T + 37
        buf = torch.full((x.shape[0], x.shape[1] + 37), float("nan"), device="cuda")
        buf[:, : x.shape[1]] = torch.tensor(x)
        xd = buf[:, : x.shape[1]]
        assert not xd.is_contiguous()
    else:
        xd = torch.tensor(x).cuda()
    return xd.requires_grad_(grad)


def run(name, grad=False):
    from golf_amd import functional as GF

    _, T, W, hop, M, centred, n_frames, _ = CASES[name]
    x = device_x(name, grad)
    out = GF.lpc_analysis(x, case(name)[1].cuda(), hop, M, centred=centred, n_frames=n_frames, return_rc=True)
    return x, out


@pytest.mark.parametrize("name", list(CASES))
def test_forward_per_frame(name):
    B, T, W, hop, M, centred, n_frames, _ = CASES[name]
    _, _, _, (rgain, ra, rrc), _ = case(name)
    _, (gain, a, rc) = run(name)
    assert gain.dtype == a.dtype == rc.dtype == torch.float32
    F = n_frames or R.n_frames_of(T, W, hop, centred)
    assert gain.shape == (B, F) and a.shape == rc.shape == (B, F, M) and ra.shape == (B, F, M)
    gain, a, rc = (t.cpu().numpy().astype(np.float64) for t in (gain, a, rc))
    assert np.isfinite(gain).all() and np.isfinite(a).all() and np.isfinite(rc).all()
    scale = np.abs(ra).max(-1)
    silent = scale == 0
    ea = np.abs(a - ra).max(-1)
    e_rc = np.abs(rc - rrc).max()
    e_gain = (np.abs(gain - rgain) / rgain).max()
    worst_a = (ea[~silent] / scale[~silent]).max()
    print(f"{name}: a {worst_a:.2e} (silent frames: {int(silent.sum())}, abs {ea[silent].max() if silent.any() else 0:.1e})  "
          f"rc {e_rc:.2e}  gain {e_gain:.2e}  max |rc| {np.abs(rrc).max():.4f}")
    assert np.all(ea[~silent] <= TOL * scale[~silent])       # every frame, relative to its own largest coefficient
    assert np.all(ea[silent] <= 1e-6)
    assert e_rc <= TOL and e_gain <= TOL
    if name in ("recipe", "order64", "from0"):
        assert silent[1].sum() >= 3 and np.abs(rrc).max() > 0.99   # the case is what it claims to be
    if name == "more_frames":
        assert silent[:, 120:].all()                              # frames past the signal see zeros


@pytest.mark.parametrize("which", COTANGENTS)
@pytest.mark.parametrize("name", list(CASES))
def test_backward(name, which):
    _, _, cot, _, g_ref = case(name)
    x, out = run(name, grad=True)
    loss = sum((o * torch.tensor(g).cuda()).sum() for o, g, nm in zip(out, cot, ("gain", "a", "rc")) if which in ("all", nm))
    loss.backward()
    g = x.grad.cpu().numpy()
    ref = g_ref[which]
    emax, el2 = rel_err(g, ref)
    print(f"{name} g_x via {which}: rel-max {emax:.2e} rel-l2 {el2:.2e}")
    assert np.isfinite(g).all()
    assert emax <= TOL and el2 <= TOL
    if CASES[name][1] == 4801:   # the silent stretch: the reference's values there, exact zeros where only silent frames reach
        assert np.abs(g[1, SILENT] - ref[1, SILENT]).max() <= TOL * np.abs(ref).max()
        zero = ref[1] == 0
        assert zero[SILENT].sum() > 100 and np.all(g[1][zero] == 0)


def test_none_cotangents_give_the_bits_of_zero_cotangents():
    """An output that nobody differentiates reaches the backward as None (a null pointer in the C call): g_x has the bits
    that explicit zero cotangents give, and a forward without rc (rc = NULL in the C call) gives the same gain, a and g_x.
    (That the null pointers are never dereferenced is what the single-cotangent cases of test_backward exercise.)"""
    from golf_amd import functional as GF

    _, _, cot, _, _ = case("odd51")
    ga = torch.tensor(cot[1]).cuda()
    x1, (gain, a, rc) = run("odd51", grad=True)
    (a * ga).sum().backward()
    x2, (gain, a, rc) = run("odd51", grad=True)
    ((a * ga).sum() + (gain * 0.0).sum() + (rc * 0.0).sum()).backward()
    assert torch.equal(x1.grad, x2.grad)
    x3 = device_x("odd51", grad=True)
    gain3, a3 = GF.lpc_analysis(x3, case("odd51")[1].cuda(), 7, 13)
    assert torch.equal(gain3, gain) and torch.equal(a3, a)
    (a3 * ga).sum().backward()
    assert torch.equal(x1.grad, x3.grad)
    x4, out = run("odd51", grad=True)
    assert torch.autograd.grad(out[0].sum(), x4, allow_unused=True)[0] is not None


def test_bit_identical_repeats():
    outs = []
    for _ in range(2):
        x, out = run("recipe", grad=True)
        sum(o.square().sum() for o in out).backward()
        outs.append((*out, x.grad))
    for u, v in zip(*outs):
        assert torch.equal(u, v)


def test_module_feeds_the_filters():
    """LPCAnalysis' outputs are the end_filter_params of both all-pole filters: reverse() gives the residual of the analysed
    audio, forward() filters an excitation, hops and lengths match."""
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import LTVMinimumPhaseFilter, LTVMinimumPhaseFilterPrecise
    from golf_amd.lpc import LPCAnalysis

    x = AudioTensor(device_x("recipe"))
    ana = LPCAnalysis(22, 240).cuda()
    gain, a = ana(x)
    assert gain.hop_length == a.hop_length == 240 and gain.shape == (2, 21) and a.shape == (2, 21, 22)
    ex = AudioTensor(torch.randn(2, 4801, generator=torch.Generator().manual_seed(1)).cuda())
    precise = LTVMinimumPhaseFilterPrecise(lpc_order=22).cuda()
    scaled, e = precise.reverse(ex, x, gain, a)
    y = precise(ex, gain, a)
    assert e.hop_length == y.hop_length == 1 and e.shape == y.shape == scaled.shape == (2, 4801)
    yf = LTVMinimumPhaseFilter(window="hanning", window_length=960, lpc_order=22).cuda()(ex, gain, a)
    assert yf.hop_length == 1 and yf.shape[0] == 2 and abs(yf.shape[1] - 4801) < 240
    for t in (scaled, e, y, yf):
        assert torch.isfinite(t.as_tensor()).all()
    # the residual of the voiced row is far below the signal: the predictor predicts
    assert e.as_tensor()[0].square().mean() < 0.1 * x.as_tensor()[0].square().mean()
    # logits() is to_logits() of the analysis
    lg, ll = ana.logits(x, 0.999)
    g2, _, rc = ana.analyse(x, return_rc=True)
    lg2, ll2 = LPCAnalysis.to_logits(g2, rc, 0.999)
    assert lg.shape == (2, 21, 1) and ll.shape == (2, 21, 22) and torch.equal(lg, lg2) and torch.equal(ll, ll2)
    assert torch.isfinite(lg).all() and torch.isfinite(ll).all()


def test_autocast_and_empty_batch():
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError

    x = device_x("odd50")
    w = case("odd50")[1].cuda()
    with torch.autocast("cuda", dtype=torch.float16):
        gain, a, rc = GF.lpc_analysis(x.half(), w, 7, 13, return_rc=True)
    assert gain.dtype == a.dtype == rc.dtype == torch.float32
    want = GF.lpc_analysis(x.half().float(), w, 7, 13, return_rc=True)
    assert all(torch.equal(u, v) for u, v in zip((gain, a, rc), want))
    with pytest.raises(GolfError):   # outside autocast a non-fp32 tensor is an error
        GF.lpc_analysis(x.half(), w, 7, 13)
    e = torch.zeros(0, 777, device="cuda", requires_grad=True)
    gain, a, rc = GF.lpc_analysis(e, w, 7, 13, return_rc=True)
    assert gain.shape == (0, 112) and a.shape == rc.shape == (0, 112, 13)
    (gain.sum() + a.sum() + rc.sum()).backward()
    assert e.grad.shape == (0, 777)


def test_refusals():
    from golf_amd import _lib
    from golf_amd import functional as GF

    x = torch.zeros(2, 1000, device="cuda")
    w = lambda n: torch.ones(n, device="cuda")
    for kw in (dict(window=w(960), hop=240, order=0), dict(window=w(960), hop=240, order=65),
               dict(window=w(22), hop=8, order=22), dict(window=w(4097), hop=240, order=22),
               dict(window=w(960), hop=0, order=22), dict(window=w(960), hop=240, order=22, n_frames=1 << 30),
               dict(window=w(960), hop=240, order=22, n_frames=0)):
        with pytest.raises(_lib.GolfError):
            GF.lpc_analysis(x, **kw)
    with pytest.raises(_lib.GolfError):
        GF.lpc_analysis(x.cpu(), w(960).cpu(), 240, 22)
    lib = _lib.load()
    ws = GF._workspace(lib.golf_lpc_analysis_workspace_bytes(2, 5, 22), "cuda")
    out = torch.empty(2, 5, 22, device="cuda")
    p = lambda t: t.data_ptr()
    for args in ((None, p(w(960)), p(out), p(out), p(ws)), (p(x), None, p(out), p(out), p(ws)),
                 (p(x), p(w(960)), None, p(out), p(ws)), (p(x), p(w(960)), p(out), None, p(ws)),
                 (p(x), p(w(960)), p(out), p(out), None)):
        xx, ww, gg, aa, wk = args
        assert lib.golf_lpc_analysis_fwd_f32(xx, 1000, ww, gg, aa, None, wk, ws.numel(), 2, 1000, 5, 22, 240, 960, -480, 1e-9,
                                             1e-12, _lib.stream_ptr()) == -1
    assert lib.golf_lpc_analysis_fwd_f32(p(x), 1000, p(w(960)), p(out), p(out), None, p(ws), 1 << 40, 1 << 16, 1000, 1 << 15,
                                         22, 240, 960, -480, 1e-9, 1e-12, _lib.stream_ptr()) == -3
    assert lib.golf_lpc_analysis_bwd_f32(None, None, None, p(x), 1000, p(w(960)), None, p(out), 1000, p(ws), ws.numel(), 2,
                                         1000, 5, 22, 240, 960, -480, 1e-9, _lib.stream_ptr()) == -1
