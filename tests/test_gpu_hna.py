"""GPU parity of the harmonic-plus-noise analysis (golf_harmonic_analysis_f32, functional.harmonic_analysis,
hna.HarmonicNoiseAnalysis) against the float64 restatement of its definition (tests/hna_ref.py, pinned on signals of known
amplitudes by tests/test_hna_host.py) on the same fp32 inputs, per frame with no frame left out.

Bars: the project's parity bar, 1e-4, in units of the frame's scale, max |x| over its window -- amplitudes; magnitudes
exp(log_mag) (a clean harmonic frame's log magnitude is the log of rounding error and cannot be held in the log domain);
phases within 1e-4 scale / amp cycles, modulo 1, where the reference's amplitude is at least 1e-2 scale; exact zeros where
the reference has exact zeros (a frame that reads no sample has S_b = 0: its log_mag is the fp32 log of eps); everything
finite.  The fp32 stand-in of tests/hna_ref.py meets the same bars on these inputs (tests/test_hna_host.py).

Largest measured errors over the cases on an MI355X, in units of the scale (profiles/hna_parity.txt has them per case, next
to the stand-in's): amplitude 2.7e-07, magnitude 3.6e-06, phase 3.8e-08."""
import math

import numpy as np
import pytest
import torch

import hna_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-4
ESTIMATOR = 1e-3   # tests/test_hna_host.py: recovery of planted amplitudes on gliding f0, in units of the largest amplitude
SIGMA = 0.05


def run(x, f0, kw, strided=False, phases=True):
    """The case through functional.harmonic_analysis; ``strided``: x and f0 as rows of wider NaN-filled buffers."""
    from golf_amd import functional as GF

    def dev(a, extra):
        if isinstance(a, torch.Tensor):
            return a
        if not strided:
            return torch.tensor(a).cuda()
        buf = torch.full((a.shape[0], a.shape[1] + extra), float("nan"), device="cuda")
        buf[:, : a.shape[1]] = torch.tensor(a)
        view = buf[:, : a.shape[1]]
        assert not view.is_contiguous() or a.shape[0] == 1
        return view

    kw = dict(kw)
    return GF.harmonic_analysis(dev(x, 37), dev(f0, 5), kw.pop("sample_rate"), kw.pop("hop"), kw.pop("K"),
                                n_mag=kw.pop("n_mag") or None, return_phases=phases, **kw)


def as_dict(out, n_mag, phases=True):
    out = out if isinstance(out, tuple) else (out,)
    assert all(t.dtype == torch.float32 and not t.requires_grad for t in out)
    arr = [t.cpu().numpy().astype(np.float64) for t in out]
    assert len(arr) == 1 + bool(phases) + bool(n_mag)
    return dict(amp=arr[0], phase=arr[1] if phases else None, log_mag=arr[-1] if n_mag else None)


def compare(name, got, ref, eps=1e-12):
    assert got["amp"].shape == ref["amp"].shape and np.isfinite(got["amp"]).all()
    if got["phase"] is None:
        got = dict(got, phase=ref["phase"])
    assert got["phase"].shape == ref["phase"].shape and np.isfinite(got["phase"]).all()
    assert ((got["phase"] >= 0) & (got["phase"] < 1)).all()
    if ref["log_mag"] is not None:
        assert got["log_mag"].shape == ref["log_mag"].shape and np.isfinite(got["log_mag"]).all()
    e_amp, e_mag, e_ph = R.errors(got, ref)
    print(f"{name}: {ref['scale'].size} frames  amp {e_amp:.2e}  mag {e_mag:.2e}  phase {e_ph:.2e}  (units of the frame's scale)")
    # exact zeros: muted harmonics, unvoiced frames, frames that read no sample
    assert (got["amp"][ref["amp"] == 0] == 0).all()
    assert (got["phase"][~ref["voiced"]] == 0).all()
    empty = ref["scale"] == 0
    if ref["log_mag"] is not None and empty.any():
        assert np.abs(got["log_mag"][empty] - 0.5 * math.log(eps)).max() <= 1e-5   # fp32 log of eps
    assert e_amp <= TOL and e_mag <= TOL and e_ph <= TOL
    return e_amp, e_mag, e_ph


@pytest.mark.parametrize("name", [n for n in R.cases() if n != "recipe"])
def test_parity_per_frame(name):
    x, f0, kw = R.cases()[name]
    compare(name, as_dict(run(x, f0, kw), kw["n_mag"]), R.reference(name))


def test_no_phase_output():
    x, f0, kw = R.cases()["K65"]
    full, part = run(x, f0, kw), run(x, f0, kw, phases=False)
    assert len(part) == 2 and torch.equal(part[0], full[0]) and torch.equal(part[1], full[2])
    compare("no phases", as_dict(part, kw["n_mag"], phases=False), R.reference("K65"))
    x, f0, kw = R.cases()["no_noise"]
    alone = run(x, f0, kw, phases=False)
    assert isinstance(alone, torch.Tensor) and torch.equal(alone, run(x, f0, kw)[0])


def test_strided_rows():
    x, f0, kw = R.cases()["hop300"]
    out = run(x, f0, kw, strided=True)
    compare("strided", as_dict(out, kw["n_mag"]), R.reference("hop300"))
    assert all(torch.equal(a, b) for a, b in zip(out, run(x, f0, kw)))


def test_outputs_overwritten_and_null_outputs_untouched():
    """Through the C ABI: outputs pre-filled with NaN are written in full; NULL phases or log_mag are not written and the
    others come out the same."""
    from golf_amd import _lib

    lib = _lib.load()
    x, f0, kw = R.cases()["K65"]
    xd, fd = torch.tensor(x).cuda(), torch.tensor(f0).cuda()
    (B, T), F, K, n_mag = x.shape, f0.shape[1], kw["K"], kw["n_mag"]

    def call(amp, phases, log_mag):
        rc = lib.golf_harmonic_analysis_f32(xd.data_ptr(), xd.stride(0), fd.data_ptr(), fd.stride(0), amp.data_ptr(),
                                            _lib.ptr(phases), _lib.ptr(log_mag), B, T, F, K, n_mag, kw["hop"], 4,
                                            2 * kw["hop"], 2048, 4 * kw["hop"], 0, kw["sample_rate"], 1e-12,
                                            _lib.stream_ptr())
        _lib.check(rc, "golf_harmonic_analysis_f32")

    def fresh():
        return [torch.full((B, F, n), float("nan"), device="cuda") for n in (K, K, n_mag, 7)]

    full = fresh()
    call(*full[:3])
    assert all(torch.isfinite(t).all() for t in full[:3]) and torch.isnan(full[3]).all()
    compare("abi", dict(amp=full[0].cpu().numpy().astype(np.float64), phase=full[1].cpu().numpy().astype(np.float64),
                        log_mag=full[2].cpu().numpy().astype(np.float64)), R.reference("K65"))
    for keep in ((1,), (2,), ()):
        part = fresh()
        call(part[0], *(part[i] if i in keep else None for i in (1, 2)))
        assert torch.equal(part[0], full[0])
        for i in (1, 2):
            assert torch.equal(part[i], full[i]) if i in keep else torch.isnan(part[i]).all()


def test_bit_reproducible_and_batch_independent():
    x, f0, kw = R.cases()["recipe"]
    xd, fd = torch.tensor(x).cuda(), torch.tensor(f0).cuda()
    first, second = run(xd, fd, kw), run(xd, fd, kw)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    for b in (0, 2, 3):
        alone = run(xd[b:b + 1], fd[b:b + 1], kw)
        assert all(torch.equal(a[0], t[b]) for a, t in zip(alone, first))
    swapped = run(xd.flip(0), fd.flip(0), kw)
    assert all(torch.equal(a.flip(0), t) for a, t in zip(swapped, first))


def test_graph_capture_replays_the_eager_result():
    x, f0, kw = R.cases()["K155"]
    xd, fd = torch.tensor(x).cuda(), torch.tensor(f0).cuda()
    eager = run(xd, fd, kw)
    sx, sf = torch.zeros_like(xd), torch.zeros_like(fd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(sx, sf, kw)                      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = run(sx, sf, kw)
    sx.copy_(xd)
    sf.copy_(fd)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, eager))


def test_autocast_grad_and_empty_batch():
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError

    x, f0, kw = R.cases()["n_mag65"]
    xd, fd = torch.tensor(x).cuda(), torch.tensor(f0).cuda()
    want = run(xd.bfloat16().float(), fd, kw)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = run(xd.bfloat16(), fd, kw)
    assert all(t.dtype == torch.float32 for t in got) and all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(GolfError, match="fp32"):
        run(xd.bfloat16(), fd, kw)
    out = run(xd.clone().requires_grad_(True), fd, kw)
    assert not any(t.requires_grad for t in out) and all(torch.equal(a, b) for a, b in zip(out, run(xd, fd, kw)))
    empty = GF.harmonic_analysis(xd[:0], fd[:0], 24000.0, 240, 8, n_mag=65, return_phases=True)
    assert [tuple(t.shape) for t in empty] == [(0, 11, 8), (0, 11, 8), (0, 11, 65)] and all(t.is_cuda for t in empty)


def test_module_on_the_recipe_shape():
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.hna import HarmonicNoiseAnalysis

    x, f0, kw = R.cases()["recipe"]
    ref = R.reference("recipe")
    xd, fd = torch.tensor(x).cuda(), torch.tensor(f0).cuda()
    assert xd.shape == (4, 4801) and fd.shape == (4, 21)
    m = HarmonicNoiseAnalysis(R.SR, R.HOP, 155, n_mag=256).cuda()
    amp, log_mag = m(AudioTensor(xd), AudioTensor(fd, R.HOP))
    assert isinstance(amp, AudioTensor) and amp.hop_length == 240 and amp.shape == (4, 21, 155)
    assert isinstance(log_mag, AudioTensor) and log_mag.hop_length == 240 and log_mag.shape == (4, 21, 256)
    three = m.analyse(xd, fd)
    compare("recipe (module)", as_dict(three, 256), ref)
    assert torch.equal(three[0], amp.as_tensor()) and torch.equal(three[2], log_mag.as_tensor())
    only = HarmonicNoiseAnalysis(R.SR, R.HOP, 155).cuda()(xd, fd)
    assert isinstance(only, AudioTensor) and torch.equal(only.as_tensor(), three[0])
    with pytest.raises(AssertionError, match="hop 1"):
        m(AudioTensor(xd, 2), fd)
    with pytest.raises(AssertionError, match="hop 240"):
        m(xd, AudioTensor(fd, 120))


def test_round_trip_on_the_packages_kernels():
    """Random smooth amplitude tracks and gliding f0 through HarmonicOscillator, analysed: the planted amplitudes come back
    on interior voiced frames within the host test's estimator bar (which the float64 oracle meets on the same audio);
    synthesise() of the analysed controls, analysed again, returns the same amplitudes within that bar; planted white noise
    comes back at the host test's level."""
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.hna import HarmonicNoiseAnalysis
    from golf_amd.synth import HarmonicOscillator

    F, K = 41, 30
    rng = np.random.default_rng(11)
    f0 = np.array([np.linspace(150.0, 250.0, F), np.linspace(110.0, 90.0, F)], np.float32)
    amps = (0.5 / np.arange(1, K + 1) * (1 + 0.2 * np.sin(rng.uniform(0, 6.28, (2, 1, K)) + 0.06 * np.arange(F)[None, :, None])))
    amps = amps.astype(np.float32)
    fd, ad = torch.tensor(f0).cuda(), torch.tensor(amps).cuda()
    x = HarmonicOscillator()(AudioTensor(fd / R.SR, R.HOP), AudioTensor(ad, R.HOP)).as_tensor()
    T = x.shape[1]
    assert T == (F - 1) * R.HOP + 1
    m = HarmonicNoiseAnalysis(R.SR, R.HOP, K, n_mag=65, smooth=4).cuda()
    top = float(amps.max())

    ref = R.analyse(x.cpu().numpy(), f0, R.SR, R.HOP, K)
    inner = np.array([[f * R.HOP - L // 2 >= 0 and f * R.HOP - L // 2 + L <= T for f, L in enumerate(row)] for row in ref["L"]])
    assert inner.sum() >= 2 * (F - 8)
    e_ref = np.abs(ref["amp"] - amps)[inner].max() / top
    got, _, log_mag = m.analyse(x, fd)
    e_got = np.abs(got.cpu().numpy() - amps)[inner].max() / top
    print(f"round trip: planted amplitudes recovered within {e_got:.2e} of the largest (float64 oracle {e_ref:.2e})")
    assert e_ref <= ESTIMATOR and e_got <= ESTIMATOR

    y = m.synthesise(fd, got)
    assert isinstance(y, AudioTensor) and y.hop_length == 1 and y.shape == x.shape
    again = m.analyse(y, AudioTensor(fd, R.HOP))[0]
    # the controls of the frames at the edges are estimates from zero-padded windows, and the bank interpolates between
    # frames: the second analysis is held on the frames whose window reads only samples made from interior frames' controls
    # (with the edge frames in, the float64 oracle on the float64 bank differs by 2.1e-2 as well; on these frames by 3.2e-4)
    deep = np.zeros_like(inner)
    for b in range(2):
        fi = np.nonzero(inner[b])[0]
        lo, hi = fi[0] * R.HOP, fi[-1] * R.HOP
        deep[b] = [f * R.HOP - L // 2 >= lo and f * R.HOP - L // 2 + L - 1 <= hi for f, L in enumerate(ref["L"][b])]
    assert deep.sum() >= 2 * (F - 12)
    e_again = (again - got).abs().cpu().numpy()[deep].max() / top
    print(f"round trip: synthesise + analyse returns the amplitudes within {e_again:.2e}")
    assert e_again <= ESTIMATOR

    noise = torch.tensor(rng.normal(0, 1, x.shape).astype(np.float32)).cuda()
    lm = m.analyse(x + SIGMA * noise, fd)[2]
    level = float(torch.exp(2 * lm.double())[torch.tensor(inner).cuda()].mean().sqrt())
    print(f"round trip: planted noise of sigma {SIGMA} comes back at {level / SIGMA:.3f} sigma")
    assert 0.7 * SIGMA <= level <= 1.05 * SIGMA

    both = m.synthesise(AudioTensor(fd, R.HOP), got, lm, noise=noise)     # harmonics + filtered noise, the shorter of the two
    assert isinstance(both, AudioTensor) and both.shape[0] == 2 and 0 < both.shape[1] <= T
    assert torch.isfinite(both.as_tensor()).all()
    drawn = m.synthesise(fd, got, lm)
    assert drawn.shape == both.shape and torch.isfinite(drawn.as_tensor()).all()
