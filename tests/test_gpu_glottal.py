"""GPU parity of the glottal-source match (golf_glottal_match_f32, functional.glottal_match, glottal.GlottalSourceAnalysis)
against the float64 restatement of its definition (tests/glottal_ref.py, pinned on pulses with a planted table position by
tests/test_glottal_host.py), per frame, fed the kernel's own harmonics so that only the match is compared.

Bars: four times the largest error of the restatement's fp32 stand-in against float64 over the same cases
(tests/test_glottal_host.py measures it and holds the stand-in to a quarter of these; profiles/glottal_parity.txt has the
figures per case): rho 1.2e-7, theta 1.2e-7 cycles, w 1.1e-4 table steps (the rounding of the outputs to fp32, the last one
at K = 1024: the kernel takes its winner again in fp64, as the stand-in does).  rho and theta are compared on every frame; w on
every frame but those where the restatement itself finds a second (k, j), more than one row from its argmax, within 1e-5 of
its maximum -- at most 2 % of a case's voiced frames (none in these cases).

The round trip through the package's oscillator and end filter is held to the restatement's own error on the same planted
case in float64 plus 25 %: the same tracks as the float64 oracle of the oscillator renders them (glottal_ref.round_trip_case,
1.43 table steps, measured by the host test; on an MI355X the round trip gives 1.43 as well).  Band-limited pulses with a
per-sample blend, the host test's signal, are another case: the oscillator interpolates the frames' blended tables over time,
a chord of the piecewise-linear blend where w crosses rows within a hop, and the restatement's error on them is 1.12."""
import numpy as np
import pytest
import torch

import glottal_ref as R

pytestmark = pytest.mark.gpu

RHO_TOL, THETA_TOL, W_TOL = 1.2e-7, 1.2e-7, 1.1e-4
TIED_CAP = 0.02


def dev(a):
    return a if isinstance(a, torch.Tensor) else torch.tensor(a).cuda()


_plans = {}


def plan_of(name):
    from golf_amd import functional as GF

    if name not in _plans:
        c = R.cases()[name]
        _plans[name] = GF.glottal_plan(dev(c["table"]), c["H"])
    return _plans[name]


def harmonics(c, x=None, f0=None):
    from golf_amd import functional as GF

    return GF.harmonic_analysis(dev(c["x"] if x is None else x), dev(c["f0"] if f0 is None else f0), c["sample_rate"],
                                c["hop"], c["H"], return_phases=True)


def run(name, f0=None, **more):
    from golf_amd import functional as GF

    c = R.cases()[name]
    f0 = dev(c["f0"] if f0 is None else f0)
    amp, ph = harmonics(c, f0=f0)
    return GF.glottal_match(amp, ph, f0, plan_of(name), c["sample_rate"], more.pop("n_phi", c["n_phi"])), (amp, ph)


def as_dict(out):
    assert all(t.dtype == torch.float32 and not t.requires_grad and t.is_contiguous() for t in out)
    return {k: t.cpu().numpy().astype(np.float64) for k, t in zip(("w", "theta", "rho"), out)}


def same(a, b):
    return (torch.isnan(a) == torch.isnan(b)).all() and torch.equal(a.nan_to_num(nan=-1.0), b.nan_to_num(nan=-1.0))


_refs = {}


def reference(name, amp, ph):
    """The float64 result of a case on the kernel's harmonics, computed once and shared."""
    if name not in _refs:
        _refs[name] = R.run(R.cases()[name], amp.cpu().numpy(), ph.cpu().numpy())
    return _refs[name]


def compare(name, got, ref, K):
    e_rho, e_theta, e_w, tied = R.errors(got, ref, K)
    print(f"{name}: {ref['w'].size} frames  rho {e_rho:.2e}  theta {e_theta:.2e} cycles  w {e_w:.2e} steps  "
          f"left out {100 * tied:.1f} %")
    ok = ~np.isnan(ref["w"])
    assert (got["theta"][ok] >= 0).all() and (got["theta"][ok] < 1).all() and (np.abs(got["rho"]) <= 1 + 1e-6).all()
    assert tied <= TIED_CAP
    assert e_rho <= RHO_TOL and e_theta <= THETA_TOL and e_w <= W_TOL


@pytest.mark.parametrize("name", list(R.cases()))
def test_parity_per_frame(name):
    out, (amp, ph) = run(name)
    compare(name, as_dict(out), reference(name, amp, ph), R.cases()[name]["table"].shape[0])


def test_cases_reach_their_edges():
    """On the kernel's own harmonics: the muted tail, the frames without an estimate, the one-sided refinements and the wrap
    of the parabola are where the cases put them."""
    refs = {}
    for name in ("H256_f400", "nyquist", "zero_frame", "edge_rows", "wrap", "recipe"):
        out, (amp, ph) = run(name)
        refs[name] = reference(name, amp, ph)
    assert (refs["H256_f400"]["Hf"] == 29).all()
    assert list(refs["nyquist"]["Hf"][0, [2, 3, 6]]) == [0, 0, 1] and np.isnan(refs["nyquist"]["w"][0, [2, 3]]).all()
    assert np.isfinite(refs["nyquist"]["w"][0, 6])
    assert np.isnan(refs["zero_frame"]["w"]).sum() >= 1 and (refs["zero_frame"]["Hf"] == 8).all()
    K = R.cases()["edge_rows"]["table"].shape[0]
    assert (R.interior(refs["edge_rows"]["k"])[0] == 0).all() and (R.interior(refs["edge_rows"]["k"])[1] == K - 1).all()
    j = R.interior(refs["wrap"]["j"])
    assert (j[0] == 0).all() and (j[1] == 63).all() and (j[2] == 0).all()
    th = R.interior(refs["wrap"]["theta"])
    assert (th[1] > 63 / 64).all() and (th[2] > 0).all() and (th[2] < 1 / 64).all()   # both neighbours across the wrap
    assert np.isnan(refs["recipe"]["w"]).sum() == 3


def test_no_estimate_is_nan_zero_zero_and_the_module_fills_it():
    from golf_amd.glottal import GlottalSourceAnalysis

    c = R.cases()["recipe"]
    (w, theta, rho), _ = run("recipe")
    none = torch.tensor(~(c["f0"] > 0)).cuda()   # the two unvoiced frames and the NaN
    assert int(none.sum()) == 3
    assert torch.isnan(w[none]).all() and (theta[none] == 0).all() and (rho[none] == 0).all()
    assert torch.isfinite(w[~none]).all() and (w[~none] >= 0).all() and (w[~none] <= 1).all()
    m = GlottalSourceAnalysis(dev(c["table"]), c["sample_rate"], c["hop"], unvoiced_weight=0.25).cuda()
    mw, mtheta, mrho = m.analyse(dev(c["x"]), dev(c["f0"]))
    assert (mw[none] == 0.25).all() and torch.equal(mw[~none], w[~none])
    assert torch.equal(mtheta, theta) and torch.equal(mrho, rho)


def test_each_output_alone_and_null_outputs_untouched():
    from golf_amd import _lib

    lib = _lib.load()
    c = R.cases()["n_phi1024"]
    full, (amp, ph) = run("n_phi1024")
    f0, p = dev(c["f0"]), plan_of("n_phi1024")
    B, F, H = amp.shape
    G, pad = B * F, 16

    def call(*outs):
        rc = lib.golf_glottal_match_f32(amp.data_ptr(), ph.data_ptr(), f0.data_ptr(), f0.stride(0), p.spectrum.data_ptr(),
                                        p.norms.data_ptr(), p.cross.data_ptr(),
                                        *[0 if o is None else o[pad:].data_ptr() for o in outs], B, F, H,
                                        p.spectrum.shape[0], c["n_phi"], c["sample_rate"], _lib.stream_ptr())
        _lib.check(rc, "golf_glottal_match_f32")

    for keep in range(3):
        bufs = [torch.full((G + 2 * pad,), float("nan"), device="cuda") for _ in range(3)]   # guard bands at both ends
        call(*[b if i == keep else None for i, b in enumerate(bufs)])
        torch.cuda.synchronize()
        for i, b in enumerate(bufs):
            assert torch.isnan(b[:pad]).all() and torch.isnan(b[G + pad:]).all()
            if i == keep:
                assert torch.equal(b[pad:G + pad].view(B, F), full[i])
            else:
                assert torch.isnan(b).all()
    with pytest.raises(_lib.GolfError, match="all NULL"):
        call(None, None, None)


def test_strided_f0_rows():
    from golf_amd import functional as GF

    c = R.cases()["recipe"]
    want, (amp, ph) = run("recipe")
    buf = torch.full((c["f0"].shape[0], c["f0"].shape[1] + 5), float("nan"), device="cuda")
    buf[:, :c["f0"].shape[1]] = dev(c["f0"])
    view = buf[:, :c["f0"].shape[1]]
    assert not view.is_contiguous()
    got = GF.glottal_match(amp, ph, view, plan_of("recipe"), c["sample_rate"], c["n_phi"])
    assert all(same(a, b) for a, b in zip(got, want))


def test_bit_reproducible_and_batch_independent():
    from golf_amd import functional as GF

    c = R.cases()["wrap"]   # three rows
    first, (amp, ph) = run("wrap")
    f0, p = dev(c["f0"]), plan_of("wrap")
    second = GF.glottal_match(amp, ph, f0, p, c["sample_rate"], c["n_phi"])
    assert all(same(a, b) for a, b in zip(first, second))
    for b in range(3):
        alone = GF.glottal_match(amp[b:b + 1], ph[b:b + 1], f0[b:b + 1], p, c["sample_rate"], c["n_phi"])
        assert all(same(a[0], t[b]) for a, t in zip(alone, first))
    swapped = GF.glottal_match(amp.flip(0), ph.flip(0), f0.flip(0), p, c["sample_rate"], c["n_phi"])
    assert all(same(a.flip(0), t) for a, t in zip(swapped, first))


def test_graph_capture_replays_the_eager_result():
    from golf_amd import functional as GF

    c = R.cases()["recipe"]
    eager, (amp, ph) = run("recipe")
    f0, p = dev(c["f0"]), plan_of("recipe")
    sa, sp, sf = torch.zeros_like(amp), torch.zeros_like(ph), torch.zeros_like(f0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        GF.glottal_match(sa, sp, sf, p, c["sample_rate"], c["n_phi"])   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = GF.glottal_match(sa, sp, sf, p, c["sample_rate"], c["n_phi"])
    sa.copy_(amp)
    sp.copy_(ph)
    sf.copy_(f0)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all(same(a, b) for a, b in zip(out, eager))


def test_autocast_grad_and_empty_batch():
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError

    c = R.cases()["n_phi1024"]
    _, (amp, ph) = run("n_phi1024")
    f0, p = dev(c["f0"]), plan_of("n_phi1024")
    args = (p, c["sample_rate"], c["n_phi"])
    want = GF.glottal_match(amp.half().float(), ph.half().float(), f0, *args)
    with torch.autocast("cuda", dtype=torch.float16):
        got = GF.glottal_match(amp.half(), ph.half(), f0, *args)
    assert all(t.dtype == torch.float32 for t in got) and all(same(a, b) for a, b in zip(got, want))
    with pytest.raises(GolfError, match="fp32"):
        GF.glottal_match(amp.half(), ph.half(), f0, *args)
    out = GF.glottal_match(amp.clone().requires_grad_(True), ph.clone().requires_grad_(True), f0, *args)
    assert not any(t.requires_grad for t in out)
    assert all(same(a, b) for a, b in zip(out, GF.glottal_match(amp, ph, f0, *args)))
    empty = GF.glottal_match(amp[:0], ph[:0], f0[:0], *args)
    assert [tuple(t.shape) for t in empty] == [(0, 9)] * 3 and all(t.is_cuda and t.dtype == torch.float32 for t in empty)
    with pytest.raises(GolfError, match="power of two"):   # refused before a launch, on the device too
        GF.glottal_match(amp, ph, f0, p, c["sample_rate"], 100)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.glottal_match(amp.cpu(), ph.cpu(), f0.cpu(), p, c["sample_rate"], c["n_phi"])


def test_module_agrees_with_the_functional():
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.glottal import GlottalSourceAnalysis
    from golf_amd.synth import GlottalFlowTable

    c = R.cases()["edge_rows"]
    (w, theta, rho), _ = run("edge_rows")
    xd, fd = dev(c["x"]), dev(c["f0"])
    m = GlottalSourceAnalysis(dev(c["table"]), c["sample_rate"], c["hop"], num_harmonics=c["H"], n_phi=c["n_phi"]).cuda()
    out = m(AudioTensor(xd), AudioTensor(fd, c["hop"]))
    assert isinstance(out, AudioTensor) and out.hop_length == c["hop"] and torch.equal(out.as_tensor(), w)
    three = m.analyse(xd, fd)
    assert torch.equal(three[0], w) and torch.equal(three[1], theta) and torch.equal(three[2], rho)
    assert torch.equal(m.logits(xd, fd), torch.logit(w.clamp(1e-6, 1 - 1e-6)))
    assert torch.isfinite(m.logits(xd, fd)).all()   # w = 0 and w = 1 are in this case
    assert not [k for k in m.state_dict() if "plan" in k or k == "table"]   # nothing of it is persistent
    with pytest.raises(AssertionError, match="hop 1"):
        m(AudioTensor(xd, 2), fd)
    with pytest.raises(AssertionError, match=f"hop {c['hop']}"):
        m(xd, AudioTensor(fd, 120))
    # a table module: its own table, followed to the device
    osc = GlottalFlowTable(table_size=10)
    mm = GlottalSourceAnalysis(osc, c["sample_rate"], c["hop"], num_harmonics=c["H"], n_phi=c["n_phi"]).cuda()
    assert mm.plan().spectrum.is_cuda and mm.plan().spectrum.shape == (10, c["H"], 2)
    assert torch.isfinite(mm(xd, fd).as_tensor()).all()


def test_plan_is_rebuilt_after_an_in_place_change_of_a_trainable_table():
    from golf_amd import functional as GF
    from golf_amd.glottal import GlottalSourceAnalysis
    from golf_amd.synth import GlottalFlowTable

    c = R.cases()["edge_rows"]
    osc = GlottalFlowTable(table_size=10, trainable=True).cuda()
    m = GlottalSourceAnalysis(osc, c["sample_rate"], c["hop"], num_harmonics=c["H"], n_phi=c["n_phi"])
    first = m.plan()
    assert m.plan().spectrum.data_ptr() == first.spectrum.data_ptr()   # cached while the table stands
    xd, fd = dev(c["x"]), dev(c["f0"])
    before = m.analyse(xd, fd)
    with torch.no_grad():
        osc.table.copy_(osc.table.flip(0))   # in place: the same storage, a new version
    second = m.plan()
    assert torch.equal(second.spectrum, first.spectrum.flip(0))
    fresh = GF.glottal_plan(osc.table, c["H"])
    assert all(torch.equal(a, b) for a, b in zip((second.spectrum, second.norms, second.cross),
                                                 (fresh.spectrum, fresh.norms, fresh.cross)))
    after = m.analyse(xd, fd)
    assert torch.allclose(after[0], 1 - before[0], atol=1e-5) and torch.allclose(after[2], before[2], atol=1e-6)


def planted_on_the_device():
    """The planted tracks of glottal_ref with a planted stable filter: (f0, w, gain, a) on the device."""
    from golf_amd import functional as GF

    f0, w = R.planted_tracks()
    F = f0.shape[1]
    g = torch.Generator().manual_seed(3)
    t = torch.linspace(0, 1, F)[None, :, None]
    rc = 0.6 * torch.tanh(torch.randn(1, 1, 8, generator=g) + 0.5 * torch.sin(6.28 * t + torch.arange(8.0)))
    gain = 1.0 + 0.3 * torch.sin(9.0 * t[..., 0])
    return dev(f0.astype(np.float32)), dev(w.astype(np.float32)), gain.cuda(), GF.rc2lpc(rc.cuda().contiguous())


def test_round_trip_on_the_packages_kernels():
    """IndexedGlottalFlowTable(oversampling=4) into LTVMinimumPhaseFilterPrecise with planted w, gain and a; residual and
    analyse return the planted w within the restatement's own error on the same tracks plus 25 %, on interior frames; and
    synthesise of the analysed w, analysed again, returns the first w within the same bar."""
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import LTVMinimumPhaseFilterPrecise
    from golf_amd.glottal import GlottalSourceAnalysis
    from golf_amd.synth import IndexedGlottalFlowTable

    f0, w, gain, a = planted_on_the_device()
    osc = IndexedGlottalFlowTable(oversampling=4).cuda()
    assert torch.equal(osc.table.cpu(), torch.tensor(R.golf_table()))
    ex = osc(AudioTensor(f0 / R.SR, R.HOP), AudioTensor(w, R.HOP))
    y = LTVMinimumPhaseFilterPrecise()(ex, AudioTensor(gain, R.HOP), AudioTensor(a, R.HOP))
    m = GlottalSourceAnalysis(osc, R.SR, R.HOP)
    e = m.residual(y, gain, a)
    assert e.shape == ex.shape
    scale = float(y.as_tensor().abs().max())   # the recursion's rounding is relative to its output
    assert float((e - ex.as_tensor()).abs().max()) <= 1e-3 * scale   # the inverse filter and the gain's upsampling undo the end filter
    w1, theta1, rho1 = m.analyse(e, f0)
    steps = osc.table.shape[0] - 1
    e_planted = float(R.interior((w1 - w).abs()).max()) * steps
    y2 = m.synthesise(f0, w1, gain, a)
    assert isinstance(y2, AudioTensor) and y2.shape == y.shape
    w2 = m.analyse(m.residual(y2, gain, a), f0)[0]
    e_again = float(R.interior((w2 - w1).abs()).max()) * steps
    bar = 1.25 * R.ROUND_TRIP_W_MAX
    print(f"round trip: planted w within {e_planted:.2f} steps, synthesise + analyse within {e_again:.2f} steps "
          f"(bar {bar:.2f}); rho >= {float(R.interior(rho1).min()):.4f}")
    assert e_planted <= bar and e_again <= bar
    assert float(R.interior(rho1).min()) >= R.RHO_BAR
    # with log_mag the noise branch is added in front of the end filter
    log_mag = torch.full((1, f0.shape[1], 65), float(np.log(1e-3)), device="cuda")
    both = m.synthesise(f0, w1, gain, a, log_mag)
    assert isinstance(both, AudioTensor) and both.shape[0] == 1 and 0 < both.shape[1] <= y.shape[1]
    assert torch.isfinite(both.as_tensor()).all()
    # a plain table tensor takes the functional oscillator: the same samples
    mt = GlottalSourceAnalysis(osc.table, R.SR, R.HOP)
    assert torch.equal(mt.synthesise(f0, w1, gain, a).as_tensor(), y2.as_tensor())
