"""GPU parity of the spectral-envelope analysis (golf_spectral_envelope_f32, functional.spectral_envelope,
envelope.SpectralEnvelopeAnalysis) against the float64 restatement of its definition (tests/env_ref.py, pinned on signals with
a planted envelope by tests/test_env_host.py) on the same fp32 inputs, per frame with no frame left out.

Bars: magnitudes exp(log_env) within the project's parity bar, 1e-4, in units of the frame's largest reference magnitude;
ceps, which lives in the log domain and has no such scale, within 3e-6 Np: 4 x the worst error of the fp32 stand-in of
tests/env_ref.py against float64 over these cases (5.3e-7 Np, case ``mixed``; tests/test_env_host.py holds the stand-in to a
quarter of the bar), rounded up to one digit -- the margin covers the difference between numpy's and the kernel's summation
order; everything finite.  The inputs carry white noise 60 dB below their rms, so that no bin is numerically empty.

A smoothing half width r < 0.5 bin, or r0 < 1 bin, cannot be reached: the window is three periods wide and must fit the
transform, so r0 = fe n / sr >= 3 and r >= 1 bin for every input the entry takes; the clamp at f0_floor is the smallest r.

Largest measured errors over the cases on an MI355X (profiles/env_parity.txt has them per case, next to the stand-in's):
magnitudes 1.5e-06 of the frame's largest, ceps 9.1e-07 Np (the frames that read no sample: one fp32 step of 0.5 log eps).
The sizes with an odd log2 n, where the kernel's ping-pong FFT ends in the other buffer: n128 magnitudes 5.0e-07, ceps
2.4e-07 Np; n512 7.1e-07, 3.9e-07 Np; n2048 8.9e-07, 2.5e-07 Np."""
import math

import numpy as np
import pytest
import torch

import env_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-4
CEPS_TOL = 3e-6
MAX_DB = 1.5    # tests/test_env_host.py: the estimator's own error on a planted envelope


def run(x, f0, kw, strided=False, **more):
    """The case through functional.spectral_envelope, every coefficient unless the case sets n_ceps; ``strided``: x and f0
    as rows of wider NaN-filled buffers."""
    from golf_amd import functional as GF

    def dev(a, extra):
        if isinstance(a, torch.Tensor):
            return a
        if not strided:
            return torch.tensor(a).cuda()
        buf = torch.full((a.shape[0], a.shape[1] + extra), float("nan"), device="cuda")
        buf[:, : a.shape[1]] = torch.tensor(a)
        view = buf[:, : a.shape[1]]
        assert not view.is_contiguous()
        return view

    kw = dict(dict(n_ceps=kw["n_fft"] // 2 + 1), **kw)
    kw.update(more)
    return GF.spectral_envelope(dev(x, 37), dev(f0, 5), kw.pop("sample_rate"), kw.pop("hop"), **kw)


def as_dict(out):
    assert all(t.dtype == torch.float32 and not t.requires_grad and t.is_contiguous() for t in out)
    return dict(log_env=out[0].cpu().numpy().astype(np.float64), ceps=out[1].cpu().numpy().astype(np.float64))


def compare(name, got, ref):
    nc = got["ceps"].shape[-1]
    assert got["log_env"].shape == ref["log_env"].shape and got["ceps"].shape == ref["ceps"].shape[:2] + (nc,)
    assert np.isfinite(got["log_env"]).all() and np.isfinite(got["ceps"]).all()
    e_env, e_ceps = R.errors(got, ref)
    print(f"{name}: {ref['voiced'].size} frames  magnitudes {e_env:.2e} of the frame's largest  ceps {e_ceps:.2e} Np")
    assert e_env <= TOL and e_ceps <= CEPS_TOL
    return e_env, e_ceps


@pytest.mark.parametrize("name", list(R.cases()))
def test_parity_per_frame(name):
    x, f0, kw = R.cases()[name]
    compare(name, as_dict(run(x, f0, kw)), R.reference(name))


def test_offset_on_voiced_frames_only():
    x, f0, kw = R.cases()["mixed"]
    with_off, without = run(x, f0, kw), run(x, f0, kw, voiced_offset=0.0)
    voiced = torch.tensor(f0 > 0).cuda()
    d_env, d_ceps = with_off[0] - without[0], with_off[1] - without[1]
    assert (d_env[~voiced] == 0).all() and (d_ceps[~voiced] == 0).all() and (d_ceps[..., 1:] == 0).all()
    assert (d_env[voiced] - R.OFFSET).abs().max() <= 2e-6 and (d_ceps[voiced][:, 0] - R.OFFSET).abs().max() <= 2e-6
    compare("no offset", as_dict(without), R.analyse(x, f0, voiced_offset=0.0, **kw))


def test_no_sample_gives_the_log_of_eps():
    x, f0, kw = R.cases()["T0"]
    env, ceps = run(x, f0, kw, voiced_offset=0.0)
    assert (env / (0.5 * math.log(1e-12)) - 1).abs().max() <= 1e-5
    assert (ceps[..., 0] / (0.5 * math.log(1e-12)) - 1).abs().max() <= 1e-5 and ceps[..., 1:].abs().max() <= 1e-6
    x, f0, kw = R.cases()["n1024"]   # frames beyond the signal read no sample either
    late = np.concatenate([f0, f0[:, -3:]], 1)
    env = run(x[:, :1000], late, kw, n_ceps=None)
    assert env.shape == (3, 12, 513) and ((env[:, 9:] - R.OFFSET) / (0.5 * math.log(1e-12)) - 1).abs().max() <= 1e-5


def test_each_output_alone():
    x, f0, kw = R.cases()["n_ceps241"]
    both = run(x, f0, kw)
    env, ceps = run(x, f0, kw, n_ceps=None), run(x, f0, kw, return_log_env=False)
    assert isinstance(env, torch.Tensor) and isinstance(ceps, torch.Tensor) and ceps.shape == (3, 9, 241)
    assert torch.equal(env, both[0]) and torch.equal(ceps, both[1])
    assert torch.equal(run(x, f0, kw, n_ceps=1)[1], both[1][..., :1])
    assert torch.equal(run(x, f0, kw, n_ceps=513)[1][..., :241], both[1])


def test_null_outputs_untouched_through_the_abi():
    from golf_amd import _lib

    lib = _lib.load()
    x, f0, kw = R.cases()["n256"]
    xd, fd = torch.tensor(x).cuda(), torch.tensor(f0).cuda()
    (B, T), F, n = x.shape, f0.shape[1], kw["n_fft"]
    lo, hi = R.defaults(kw["sample_rate"], n)

    def call(env, ceps, n_ceps):
        rc = lib.golf_spectral_envelope_f32(xd.data_ptr(), xd.stride(0), fd.data_ptr(), fd.stride(0), _lib.ptr(env),
                                            _lib.ptr(ceps), B, T, F, n, n_ceps, kw["hop"], kw["sample_rate"], lo, hi,
                                            kw["unvoiced_f0"], -0.15, 1e-12, R.OFFSET, _lib.stream_ptr())
        _lib.check(rc, "golf_spectral_envelope_f32")

    def fresh():
        return [torch.full((B, F, w), float("nan"), device="cuda") for w in (n // 2 + 1, 40, 7)]

    full = fresh()
    call(full[0], full[1], 40)
    assert torch.isfinite(full[0]).all() and torch.isfinite(full[1]).all() and torch.isnan(full[2]).all()
    compare("abi", as_dict(full[:2]), R.reference("n256"))
    part = fresh()
    call(part[0], None, 0)
    assert torch.equal(part[0], full[0]) and torch.isnan(part[1]).all()
    part = fresh()
    call(None, part[1], 40)
    assert torch.equal(part[1], full[1]) and torch.isnan(part[0]).all()


def test_strided_rows():
    x, f0, kw = R.cases()["mixed"]
    out = run(x, f0, kw, strided=True)
    compare("strided", as_dict(out), R.reference("mixed"))
    assert all(torch.equal(a, b) for a, b in zip(out, run(x, f0, kw)))


def test_bit_reproducible_and_batch_independent():
    x, f0, kw = R.cases()["mixed"]
    xd, fd = torch.tensor(x).cuda(), torch.tensor(f0).cuda()
    first, second = run(xd, fd, kw), run(xd, fd, kw)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    for b in range(3):
        alone = run(xd[b:b + 1], fd[b:b + 1], kw)
        assert all(torch.equal(a[0], t[b]) for a, t in zip(alone, first))
    swapped = run(xd.flip(0), fd.flip(0), kw)
    assert all(torch.equal(a.flip(0), t) for a, t in zip(swapped, first))


def test_graph_capture_replays_the_eager_result():
    x, f0, kw = R.cases()["n1024"]
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

    x, f0, kw = R.cases()["n1024"]
    xd, fd = torch.tensor(x).cuda(), torch.tensor(f0).cuda()
    want = run(xd.half().float(), fd, kw)
    with torch.autocast("cuda", dtype=torch.float16):
        got = run(xd.half(), fd, kw)
    assert all(t.dtype == torch.float32 for t in got) and all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(GolfError, match="fp32"):
        run(xd.half(), fd, kw)
    out = run(xd.clone().requires_grad_(True), fd, kw)
    assert not any(t.requires_grad for t in out) and all(torch.equal(a, b) for a, b in zip(out, run(xd, fd, kw)))
    empty = GF.spectral_envelope(xd[:0], fd[:0], 24000.0, 240, n_ceps=241)
    assert [tuple(t.shape) for t in empty] == [(0, 9, 513), (0, 9, 241)] and all(t.is_cuda for t in empty)
    assert GF.spectral_envelope(xd[:0], fd[:0], 24000.0, 240).shape == (0, 9, 513)
    with pytest.raises(GolfError, match="longest window"):   # refused before a launch, on the device too
        GF.spectral_envelope(xd, fd, 24000.0, 240, f0_floor=60.0)


def test_module_agrees_with_the_functional():
    from golf_amd import functional as GF
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.envelope import SpectralEnvelopeAnalysis

    x, f0, kw = R.cases()["n1024"]
    xd, fd = torch.tensor(x).cuda(), torch.tensor(f0).cuda()
    env, ceps = GF.spectral_envelope(xd, fd, R.SR, R.HOP, n_ceps=241)
    m = SpectralEnvelopeAnalysis(R.SR, R.HOP, filter_order=240).cuda()
    out = m(AudioTensor(xd), AudioTensor(fd, R.HOP))
    assert isinstance(out, AudioTensor) and out.hop_length == 240 and torch.equal(out.as_tensor(), ceps)
    two = m.analyse(xd, fd)
    assert torch.equal(two[0], env) and torch.equal(two[1], ceps)
    plain = SpectralEnvelopeAnalysis(R.SR, R.HOP).cuda()
    out = plain(xd, fd)
    assert isinstance(out, AudioTensor) and out.hop_length == 240 and torch.equal(out.as_tensor(), env)
    assert plain.analyse(xd, fd)[1].shape == (3, 9, 513)
    rows = m.response_rows(xd, fd)
    assert torch.equal(rows, torch.exp(env))
    # the rows feed the frame filter as they are: fp32, contiguous, (B, F, n/2 + 1)
    assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.shape == (3, 9, 513)
    window = torch.hann_window(1024, device="cuda")
    y = GF.stft_filter_frames(xd, rows, window, R.HOP)
    assert y.shape == (3, 8 * R.HOP) and torch.isfinite(y).all()
    with pytest.raises(AssertionError, match="hop 1"):
        m(AudioTensor(xd, 2), fd)
    with pytest.raises(AssertionError, match="hop 240"):
        m(xd, AudioTensor(fd, 120))


def test_copy_synthesis_on_the_packages_kernels():
    """AdditivePulseTrain through LTVCepFilter with a planted cepstrum, analysed: the planted envelope comes back within the
    estimator's bar on interior frames; synthesise() of the analysed ceps, analysed again, returns the first analysis's
    log_env within that bar; with log_mag the noise branch is added and the result is the shorter of the two."""
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.envelope import SpectralEnvelopeAnalysis

    F = 41
    f0 = np.array([np.linspace(150.0, 250.0, F), np.full(F, 120.0)], np.float32)
    fd = torch.tensor(f0).cuda()
    m = SpectralEnvelopeAnalysis(R.SR, R.HOP, filter_order=240).cuda()
    planted = torch.zeros(2, F, 241, device="cuda")
    planted[..., :7] = torch.tensor(R.PLANTED_CEPS, dtype=torch.float32).cuda()
    x = m.synthesise(fd, planted)
    assert isinstance(x, AudioTensor) and x.hop_length == 1 and x.shape == (2, (F - 1) * R.HOP)
    env, ceps = m.analyse(x, fd)
    want = R.log_response(R.PLANTED_CEPS, np.arange(487) / 1024.0)
    e_planted = R.DB * np.abs(env[:, 5:-5, :487].cpu().numpy() - want).max()
    y = m.synthesise(AudioTensor(fd, R.HOP), ceps)
    again = m.analyse(y, fd)[0]
    e_again = R.DB * float((again - env)[:, 5:-5, :487].abs().max())
    print(f"copy-synthesis: planted envelope within {e_planted:.2f} dB, synthesise + analyse within {e_again:.2f} dB")
    assert e_planted <= MAX_DB and e_again <= MAX_DB
    log_mag = torch.full((2, F, 65), math.log(1e-2), device="cuda")
    both = m.synthesise(fd, ceps, log_mag)
    assert isinstance(both, AudioTensor) and both.shape[0] == 2 and 0 < both.shape[1] <= y.shape[1]
    assert torch.isfinite(both.as_tensor()).all()
    noise = torch.randn(2, (F - 1) * R.HOP + 1, device="cuda")
    fixed = m.synthesise(fd, ceps, log_mag, noise=AudioTensor(noise))
    assert torch.equal(fixed.as_tensor(), m.synthesise(fd, ceps, log_mag, noise=noise).as_tensor())
