"""GPU: the source-compensated LPC analysis (golf_lpc_source_filter_f32, functional.source_filter_lpc,
lpc.SourceFilterLPCAnalysis, analysis_stream.SourceFilterLPCStream) against the float64 restatement of its definition
(tests/sflpc_ref.py, pinned by tests/test_sflpc_host.py) on the same fp32 inputs.

Audio: seeded noise through the all-pole filters of tests/golden/g25 (lpc_analysis_ref.speech_like), B = 3: row 1 is all
zeros, row 2 has one NaN sample.  Bars: those of tests/test_gpu_lpc_analysis.py, TOL = 1e-4 per frame with no frame left out
-- a and source: rel-max over the frame's coefficients (1e-6 absolute where the reference is exactly 0: silent frames), rc:
absolute, gain: relative.  The frames that read the NaN sample are NaN in a, rc and source, in the reference and on the
device, and no other frame is; their gain is max(NaN, 0) = 0 on the device, as golf_lpc_analysis_fwd_f32 gives it, and is not
compared.  Worst values reached: profiles/sflpc_parity.txt."""
import functools

import numpy as np
import pytest
import torch

import lpc_analysis_ref as L
import sflpc_ref as S
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TOL = 1e-4

# name -> (M, Q, I, preemphasis, W, hop, T, centred): the smallest shapes that reach each branch
CASES = {
    "default": (22, 4, 2, None, 960, 240, 2400, True),
    "fixed0.97": (22, 4, 2, 0.97, 960, 240, 2400, True),
    "second_pass": (7, 1, 0, None, 64, 16, 300, True),        # J + 1 = 9: one lag into the second pass
    "Q=M": (8, 8, 1, None, 64, 16, 300, True),
    "smallest_W": (1, 1, 1, None, 3, 1, 17, True),
    "73_lags": (64, 8, 2, None, 256, 64, 1000, True),         # more lags than lanes, 65 coefficients
    "largest": (22, 16, 8, None, 4096, 1024, 6000, True),     # two-wave workgroups, the most stages
    "odd_W_from0": (10, 4, 2, None, 481, 100, 1500, False),
    "hop>W": (10, 4, 2, None, 64, 100, 700, True),
    "T<W": (22, 4, 2, None, 960, 240, 100, True),
    "15_frames": (10, 4, 2, None, 64, 16, 64, True),          # B F = 3 * 5: the last workgroup has one idle wave
    "F=1": (10, 4, 2, None, 64, 16, 40, False),
}
NAN_ROW = 2


def _golden(name):
    import os

    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


@functools.lru_cache(maxsize=None)
def audio(T):
    """(3, T) fp32: speech-like rows, row 1 all zeros, one NaN in row 2 (at 2 T / 3); computed once, never changed."""
    x = L.speech_like(_golden, (0, 9, 4), T, hop=max(240, -(-T // 20)), seed=T).astype(np.float32)
    assert x.shape == (3, T)
    x[1] = 0.0
    x[NAN_ROW, 2 * T // 3] = np.nan
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def case(name):
    """(x fp32, window, the float64 reference (gain, a, rc, source) as numpy) of one case."""
    M, Q, I, pre, W, hop, T, centred = CASES[name]
    x, window = audio(T), torch.hann_window(W)
    ref = tuple(t.numpy() for t in S.analysis(x, window, hop, M, Q, I, pre, centred=centred))
    for arr in ref:
        arr.setflags(write=False)
    return x, window, ref


def run(name, x=None, window=None, **kw):
    from golf_amd import functional as GF

    M, Q, I, pre, W, hop, T, centred = CASES[name]
    x = torch.tensor(case(name)[0]).cuda() if x is None else x
    window = case(name)[1].cuda() if window is None else window
    kw = dict(dict(return_rc=True, return_source=True, centred=centred), **kw)
    return GF.source_filter_lpc(x, window, hop, M, Q, I, pre, **kw)


def same(u, v):
    """The same bits, NaNs included."""
    return u.shape == v.shape and torch.equal(u.contiguous().view(torch.int32), v.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", list(CASES))
def test_parity_per_frame(name):
    M, Q, I, pre, W, hop, T, centred = CASES[name]
    x, _, (rgain, ra, rrc, rsrc) = case(name)
    gain, a, rc, src = run(name)
    F = L.n_frames_of(T, W, hop, centred)
    assert gain.dtype == a.dtype == rc.dtype == src.dtype == torch.float32
    assert gain.shape == (3, F) and a.shape == rc.shape == (3, F, M) and src.shape == (3, F, Q) and rsrc.shape == (3, F, Q)
    assert not any(t.requires_grad for t in (gain, a, rc, src))
    gain, a, rc, src = (t.cpu().numpy().astype(np.float64) for t in (gain, a, rc, src))
    # the frames that read the NaN sample, from the frame grid alone
    o = np.arange(F) * hop - (W // 2 if centred else 0)
    t_nan = 2 * T // 3
    bad = np.zeros((3, F), bool)
    bad[NAN_ROW] = (o <= t_nan) & (t_nan < o + W)
    for got, ref in ((a, ra), (rc, rrc), (src, rsrc)):   # (with I = 0 the padding of source is 0 in those frames too)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isnan(ref).any(-1), bad)
    assert np.array_equal(np.isnan(a).all(-1), bad) and np.array_equal(np.isnan(rgain), bad)
    ok = ~bad
    assert np.isfinite(gain[ok]).all()
    gain[bad], rgain = 1.0, np.where(bad, 1.0, rgain)   # not compared
    worst = {}
    for nm, got, ref in (("a", a, ra), ("source", src, rsrc)):
        scale = np.abs(ref).max(-1)
        err = np.abs(got - ref).max(-1)
        zero = ok & (scale == 0)
        live = ok & (scale > 0)
        worst[nm] = (err[live] / scale[live]).max(initial=0.0)
        assert np.all(err[live] <= TOL * scale[live]), (nm, worst[nm])   # every frame, relative to its own largest coefficient
        assert np.all(err[zero] <= 1e-6)
        if nm == "a":   # the speech row has a model (W = 3: but for the last two frames, at the end); the silent row gives a = 0
            assert live[0].sum() >= F - 2   # (behind a fixed pre-emphasis the regularised r[0] is coloured by it instead)
            assert zero[1].all() if pre is None else live[1].all()
    e_rc = np.abs(rc - rrc)[ok].max()
    e_gain = (np.abs(gain - rgain) / rgain)[ok].max()
    print(f"{name}: a {worst['a']:.2e}  source {worst['source']:.2e}  rc {e_rc:.2e}  gain {e_gain:.2e}  "
          f"max |rc| {np.abs(rrc[ok]).max():.4f}  NaN frames {int(bad.sum())} of {3 * F}")
    assert e_rc <= TOL and e_gain <= TOL
    assert np.abs(rc[ok]).max() < 1.0
    if I == 0:
        assert np.all(src[ok][:, 1:] == 0)   # zero padded


def test_without_a_source_model_it_is_lpc_analysis():
    """preemphasis=0, iterations=0: a and rc have the bits of lpc_analysis; the gain, (r o a)[0] against E_M in fp64, is
    within one fp32 ulp."""
    from golf_amd import functional as GF

    for T, W, hop, M in ((2400, 960, 240, 22), (1000, 256, 64, 64), (300, 51, 7, 13)):
        x, w = torch.tensor(audio(T)[:2]).cuda(), torch.hann_window(W).cuda()   # the rows without a NaN
        gain0, a0, rc0 = GF.lpc_analysis(x, w, hop, M, return_rc=True)
        gain, a, rc, src = GF.source_filter_lpc(x, w, hop, M, 4, 0, 0.0, return_rc=True, return_source=True)
        assert torch.equal(a, a0) and torch.equal(rc, rc0) and torch.all(src == 0)
        ulps = (gain.view(torch.int32) - gain0.view(torch.int32)).abs().max().item()
        print(f"T={T} W={W} M={M}: gain differs by at most {ulps} ulp")
        assert ulps <= 1


def test_reproducible_and_independent_of_the_batch():
    first, again = run("default"), run("default")
    assert all(same(u, v) for u, v in zip(first, again))
    x = torch.tensor(case("default")[0]).cuda()
    for b in range(3):   # a row alone is the row in its batch
        assert all(same(u[0], v[b]) for u, v in zip(run("default", x[b:b + 1]), first))
    wide = torch.full((3, x.shape[1] + 37), 7.0, device="cuda")   # rows of a wider buffer, read in place
    wide[:, 5:5 + x.shape[1]] = x
    xs = wide[:, 5:5 + x.shape[1]]
    assert not xs.is_contiguous()
    assert all(same(u, v) for u, v in zip(run("default", xs), first))
    assert all(same(u, v) for u, v in zip(run("default", return_rc=False, return_source=False), first[:2]))


def _stream_cases(x, module, blocks, **kw):
    """Push x through a fresh stream in blocks of each size; -> per block size the concatenated plain results."""
    from golf_amd.analysis_stream import open_analysis_stream

    out = []
    for n in blocks:
        st = open_analysis_stream(module, x.shape[0], **kw)
        parts = [st.push_all(x[:, t:t + n]) for t in range(0, x.shape[1], n)] + [st.finish_all()]
        out.append(tuple(torch.cat([p[j] for p in parts], 1) for j in range(len(parts[0]))))
    return out


@pytest.mark.parametrize("centred,W,hop", [(True, 240, 60), (False, 240, 60), (True, 48, 60)])   # the last: hop > W
def test_stream_is_the_one_shot_bit_for_bit(centred, W, hop):
    from golf_amd import analysis_stream as AS
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.lpc import SourceFilterLPCAnalysis

    T = 1500
    x = torch.tensor(audio(T)[[0, NAN_ROW]]).cuda()
    m = SourceFilterLPCAnalysis(10, hop, W, centred=centred).cuda()
    want = m.analyse(x, return_rc=True, return_source=True)
    assert want[0].shape == (2, L.n_frames_of(T, W, hop, centred)) and want[3].shape[2] == 4
    for n, got in zip((1, 37, 60, 245, T), _stream_cases(x, m, (1, 37, 60, 245, T), return_rc=True, return_source=True)):
        assert len(got) == 4 and all(same(u, v) for u, v in zip(got, want)), n
    st = AS.open_analysis_stream(m, 2)
    assert type(st) is AS.SourceFilterLPCStream
    # two utterances back to back through one stream, as AudioTensors: (gain, a) of forward
    for xx in (x, x[:, 333:1200]):
        parts = [st.push(AudioTensor(xx[:, t:t + 245])) for t in range(0, xx.shape[1], 245)] + [st.finish()]
        assert all(len(p) == 2 and p[0].hop_length == p[1].hop_length == hop for p in parts)
        gain, a = m(AudioTensor(xx))
        assert same(torch.cat([p[0].as_tensor() for p in parts], 1), gain.as_tensor())
        assert same(torch.cat([p[1].as_tensor() for p in parts], 1), a.as_tensor())


def test_module_feeds_the_residual_and_the_filter():
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import LTVMinimumPhaseFilterPrecise
    from golf_amd.glottal import GlottalSourceAnalysis
    from golf_amd.lpc import LPCAnalysis, SourceFilterLPCAnalysis

    x = AudioTensor(torch.tensor(audio(2400)[:1]).cuda())
    ana = SourceFilterLPCAnalysis(22, 240).cuda()
    gain, a = ana(x)
    assert gain.hop_length == a.hop_length == 240 and gain.shape == (1, 11) and a.shape == (1, 11, 22)
    table = torch.tensor(__import__("glottal_ref").golf_table())
    glo = GlottalSourceAnalysis(table, 24000.0, 240).cuda()
    e = glo.residual_fused(x, gain, a)
    assert e.shape == (1, 2400) and torch.isfinite(e).all()
    assert 0.5 < e[:, 480:-480].square().mean().sqrt() < 2.0   # unit local power, by the definition of the gain
    precise = LTVMinimumPhaseFilterPrecise(lpc_order=22).cuda()
    ex = AudioTensor(torch.randn(1, 2400, generator=torch.Generator().manual_seed(1)).cuda())
    scaled, e2 = precise.reverse(ex, x, gain, a)
    assert e2.hop_length == 1 and e2.shape == scaled.shape and torch.isfinite(e2.as_tensor()).all()
    lg, ll = ana.logits(x, 0.999)
    g2, _, rc = ana.analyse(x, return_rc=True)
    lg2, ll2 = LPCAnalysis.to_logits(g2, rc, 0.999)
    assert lg.shape == (1, 11, 1) and ll.shape == (1, 11, 22) and torch.equal(lg, lg2) and torch.equal(ll, ll2)


def test_worth_on_the_planted_case_on_the_device():
    """The planted construction of tests/test_sflpc_host.py through the device's own modules, SourceFilterLPCAnalysis ->
    residual_fused -> GlottalSourceAnalysis: the rms error of w is strictly below the same chain with LPCAnalysis, at both
    table positions."""
    import glottal_ref as G
    from golf_amd.glottal import GlottalSourceAnalysis
    from golf_amd.lpc import LPCAnalysis, SourceFilterLPCAnalysis

    glo = GlottalSourceAnalysis(torch.tensor(G.golf_table()), G.SR, G.HOP).cuda()
    for w0 in (0.3, 0.7):
        pl = S.planted(w0)
        case_, y = pl["case"], torch.tensor(pl["y"][None].astype(np.float32)).cuda()
        f0 = torch.tensor(case_["f0"]).cuda()
        rms = {}
        for name, ana in (("plain", LPCAnalysis(S.ORDER, G.HOP)), ("source-filter", SourceFilterLPCAnalysis(S.ORDER, G.HOP))):
            gain, a = ana.cuda().analyse(y)
            w = glo.analyse(glo.residual_fused(y, gain, a), f0)[0].cpu().numpy().astype(np.float64)
            dw = G.interior(np.abs(w - case_["w"])) * (case_["table"].shape[0] - 1)
            rms[name] = float(np.sqrt((dw ** 2).mean()))
        print(f"w = {w0}: rms error of w in table steps: {rms}")
        assert rms["source-filter"] < rms["plain"]


def test_autocast_empty_batch_and_no_grad():
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError

    x = torch.tensor(audio(300)[:2]).cuda()
    w = torch.hann_window(64).cuda()
    with torch.autocast("cuda", dtype=torch.float16):
        got = GF.source_filter_lpc(x.half(), w, 16, 10, return_rc=True, return_source=True)
    assert all(t.dtype == torch.float32 for t in got)
    want = GF.source_filter_lpc(x.half().float(), w, 16, 10, return_rc=True, return_source=True)
    assert all(torch.equal(u, v) for u, v in zip(got, want))
    with pytest.raises(GolfError):   # outside autocast a non-fp32 tensor is an error
        GF.source_filter_lpc(x.half(), w, 16, 10)
    e = torch.zeros(0, 300, device="cuda")
    gain, a, rc, src = GF.source_filter_lpc(e, w, 16, 10, return_rc=True, return_source=True)
    assert gain.shape == (0, 19) and a.shape == rc.shape == (0, 19, 10) and src.shape == (0, 19, 4)
    out = GF.source_filter_lpc(x.clone().requires_grad_(True), w, 16, 10, return_rc=True, return_source=True)
    assert len(out) == 4 and not any(t.requires_grad for t in out)
    assert all(torch.equal(u, v) for u, v in zip(out, GF.source_filter_lpc(x, w, 16, 10, return_rc=True, return_source=True)))


def test_graph_capture_replays_the_eager_bits():
    xd, w = torch.tensor(case("default")[0]).cuda(), case("default")[1].cuda()   # (no copy from the host inside the capture)
    eager = run("default", xd, w)
    static = torch.zeros_like(xd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run("default", static, w)                   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = run("default", static, w)
    static.copy_(xd)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all(same(u, v) for u, v in zip(out, eager))


def test_refusals():
    """Every refusal, through the C entry with its return code and through the functional; nothing is launched."""
    from golf_amd import _lib
    from golf_amd import functional as GF

    x = torch.zeros(2, 1000, device="cuda")
    w = lambda n: torch.ones(n, device="cuda")
    for kw in (dict(window=w(960), order=0), dict(window=w(960), order=65), dict(window=w(960), source_order=0),
               dict(window=w(960), source_order=17), dict(window=w(960), iterations=-1), dict(window=w(960), iterations=9),
               dict(window=w(26)), dict(window=w(4097)), dict(window=w(960), hop=0), dict(window=w(960), n_frames=1 << 30),
               dict(window=w(960), n_frames=0), dict(window=w(960), preemphasis=1.0), dict(window=w(960), preemphasis=-1.0),
               dict(window=w(960), preemphasis=float("nan")), dict(window=w(960), preemphasis=float("inf"))):
        with pytest.raises(_lib.GolfError):
            GF.source_filter_lpc(x, **dict(dict(hop=240, order=22), **kw))
    with pytest.raises(_lib.GolfError):
        GF.source_filter_lpc(x.cpu(), w(960).cpu(), 240, 22)
    with pytest.raises(_lib.GolfError):
        GF.source_filter_lpc(x[0], w(960), 240, 22)
    lib = _lib.load()
    gain, a, win = torch.empty(2, 5, device="cuda"), torch.empty(2, 5, 22, device="cuda"), w(960)
    p = lambda t: None if t is None else t.data_ptr()

    def call(B=2, T=1000, F=5, M=22, Q=4, I=2, adaptive=1, pre=0.0, hop=240, W=960, ptrs=(x, win, gain, a)):
        xx, ww, gg, aa = ptrs
        return lib.golf_lpc_source_filter_f32(p(xx), 1000, p(ww), p(gg), p(aa), None, None, B, T, F, M, Q, I, adaptive, pre, hop,
                                              W, -(W // 2), 1e-9, 1e-12, _lib.stream_ptr())

    EINVAL, EUNSUPPORTED = -1, -3
    for ptrs in ((None, win, gain, a), (x, None, gain, a), (x, win, None, a), (x, win, gain, None)):
        assert call(ptrs=ptrs) == EINVAL
    for pre in (1.0, -1.0, float("nan"), float("inf")):
        assert call(adaptive=0, pre=pre) == EINVAL
    for kw in (dict(M=0), dict(M=65), dict(Q=0), dict(Q=17), dict(I=-1), dict(I=9), dict(W=26), dict(W=4097), dict(hop=0),
               dict(B=1 << 16, F=1 << 15)):
        assert call(**kw) == EUNSUPPORTED, kw
    assert call(B=0) == 0
    gain.fill_(-7.0)
    a.fill_(-7.0)
    assert call() == 0   # the arguments above were one step from a call that runs
    torch.cuda.synchronize()
    assert (gain > 0).all() and (a == 0).all()
