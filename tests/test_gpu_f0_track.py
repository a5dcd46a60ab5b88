"""GPU parity of the f0 tracker (golf_f0_candidates_f32, golf_f0_viterbi_f32, functional.f0_candidates / f0_viterbi / f0_track,
f0.F0Tracker) against the float64 restatement of its definition (tests/f0_track_ref.py, pinned by
tests/test_f0_track_host.py) on the same fp32 inputs.

Bars.  Candidates: slots are matched in order; a frame whose pattern of present slots differs, or one of whose periods lies
more than a sample from the reference's lag, is a flip, a case may have them in 1 % of its frames, rounded down, and every
other frame is held to 1e-4 (period relative, ap absolute) with its absent slots exactly 0 / +inf.  Path: the states equal
the reference's exactly wherever the reference's margin is >= 1e-6 (asserted by the host test: the kernel's float64 costs
differ from the reference's by roundoff, nine orders below), and its cost, evaluated by the reference, is within 1e-9 of the
optimum whatever the ties."""
import numpy as np
import pytest
import torch

import f0_ref as R
import f0_track_ref as TR

pytestmark = pytest.mark.gpu

TOL = 1e-4


def freqs(kw):
    """The frequencies that give the explicit lags of a case."""
    from golf_amd import functional as GF

    sr = kw["sample_rate"]
    f0_max, f0_min = sr / (kw["tau_min"] + 0.5), sr / (kw["tau_max"] - 0.5)
    assert GF.f0_lags(sr, f0_min, f0_max, kw["W"]) == (kw["tau_min"], kw["tau_max"], kw["W"])
    return f0_min, f0_max


def dev(x, strided=False):
    if isinstance(x, torch.Tensor):
        return x
    if strided:   # rows of a wider buffer: unit inner stride, row stride T + 37
        buf = torch.full((x.shape[0], x.shape[1] + 37), float("nan"), device="cuda")
        buf[:, : x.shape[1]] = torch.tensor(x)
        xd = buf[:, : x.shape[1]]
        assert not xd.is_contiguous()
        return xd
    return torch.tensor(x).cuda()


def run_cand(x, kw, K=7, strided=False):
    from golf_amd import functional as GF

    f0_min, f0_max = freqs(kw)
    return GF.f0_candidates(dev(x, strided), kw["sample_rate"], kw["hop"], f0_min, f0_max, kw["W"], K, kw.get("rms_floor", 0.0),
                            centred=kw.get("centred", True), n_frames=kw.get("F"))


def run_track(x, kw, K=7, **more):
    from golf_amd import functional as GF

    f0_min, f0_max = freqs(kw)
    return GF.f0_track(dev(x), kw["sample_rate"], kw["hop"], f0_min, f0_max, kw["W"], K, kw.get("rms_floor", 0.0),
                       centred=kw.get("centred", True), n_frames=kw.get("F"), return_all=True, **more)


def compare_candidates(name, out, ref):
    period, ap = (t.cpu().numpy().astype(np.float64) for t in out)
    assert period.shape == ap.shape == ref["period"].shape
    there = ref["lag"] >= 0
    got = (period > 0) & (ap < np.inf)
    off = there & got & (np.abs(period - ref["lag"]) > 1.0)
    flip = (got != there).any(-1) | off.any(-1)
    ok = ~flip[..., None] & there
    gone = ~flip[..., None] & ~there
    e_p = (np.abs(period[ok] - ref["period"][ok]) / ref["period"][ok]).max() if ok.any() else 0.0
    e_ap = np.abs(ap[ok] - ref["ap"][ok]).max() if ok.any() else 0.0
    print(f"{name}: {flip.size} frames, {int(flip.sum())} flips; period {e_p:.2e}  ap {e_ap:.2e}")
    assert int(flip.sum()) <= flip.size // 100
    assert (period[gone] == 0).all() and (ap[gone] == np.inf).all()
    assert e_p <= TOL and e_ap <= TOL


def test_the_cases_cover_the_selection():
    """In the reference, before anything is compared: frames without a minimum, with fewer than K, with more than K, and
    with a minimum at tau_max."""
    none = fewer = more = at_end = False
    for name in TR.cand_case_names():
        kw = R.cases()[name][1]
        for K in (1, 3, 7):
            ref = TR.cand_reference(name, K)
            none |= bool((ref["n_minima"] == 0).any())
            fewer |= bool(((ref["n_minima"] > 0) & (ref["n_minima"] < K)).any())
            more |= bool((ref["n_minima"] > K).any())
            at_end |= bool((ref["lag"] == kw["tau_max"]).any())
    assert none and fewer and more and at_end
    assert {f"tau_max{t}" for t in (63, 64, 65, 255, 256, 257)} <= set(TR.cand_case_names())
    assert (TR.cand_reference("quiet_floor", 7)["lag"] == -1).all() and (TR.cand_reference("quiet_floor", 7)["n_minima"] > 0).any()


@pytest.mark.parametrize("K", (1, 3, 7))
@pytest.mark.parametrize("name", TR.cand_case_names())
def test_candidate_parity(name, K):
    x, kw = R.cases()[name]
    out = run_cand(x, kw, K)
    assert all(t.dtype == torch.float32 and not t.requires_grad and t.shape[-1] == K for t in out)
    compare_candidates(f"{name} K={K}", out, TR.cand_reference(name, K))


@pytest.mark.parametrize("name", ("recipe", "small50", "tau_max257", "star_at_tau_max", "fallback", "first_at_tau_min"))
def test_candidates_agree_bitwise_with_f0_yin(name):
    """Where YIN's tau* is among the kept lags (so says the reference), that slot's period and ap are golf_f0_yin_f32's to
    the bit: both kernels refine from one d'."""
    from golf_amd import functional as GF

    x, kw = R.cases()[name]
    ref = TR.cand_reference(name, 7)
    f0_min, f0_max = freqs(kw)
    xd = dev(x)
    _, period, ap = GF.f0_yin(xd, kw["sample_rate"], kw["hop"], f0_min, f0_max, kw["W"], kw.get("threshold", 0.15),
                              centred=kw.get("centred", True), n_frames=kw.get("F"), return_all=True)
    cp, ca = run_cand(xd, kw, 7)
    hit = torch.tensor(ref["lag"] == ref["yin"]["tau"][..., None]).cuda()
    frames = hit.any(-1)
    print(f"{name}: tau* is kept in {int(frames.sum())} of {frames.numel()} frames")
    assert frames.sum() >= frames.numel() // 2
    assert torch.equal(cp[hit], period[frames]) and torch.equal(ca[hit], ap[frames])


def run_path(p, a, **kw):
    from golf_amd import functional as GF

    return GF.f0_viterbi(torch.tensor(p).cuda(), torch.tensor(a).cuda(), 24000.0, 24.0, return_state=True, **kw)


@pytest.mark.parametrize("F,K", TR.PATH_SHAPES + TR.PATH_SHAPES_SWITCH)
def test_path_kernel_alone(F, K):
    from golf_amd import _lib

    seed, p, a, ref = TR.path_seed(F, K)
    assert ref["margin"] >= 1e-6
    needs_ws = _lib.load().golf_f0_viterbi_workspace_bytes(TR.PATH_B, F, K) > 0
    assert needs_ws == (F > TR.LDS_FRAMES)
    f0, state = run_path(p, a)
    assert f0.dtype == torch.float32 and state.dtype == torch.int32 and f0.shape == state.shape == (TR.PATH_B, F)
    f0, state = f0.cpu().numpy().astype(np.float64), state.cpu().numpy()
    costs = [TR.path_cost(state[b], p[b], a[b], 24.0, **TR.COSTS) for b in range(TR.PATH_B)]
    print(f"F = {F}, K = {K}: {int((state != ref['state']).sum())} states differ; cost above the optimum "
          f"{max(c - r for c, r in zip(costs, ref['cost'])):.2e}")
    assert all(c <= r + 1e-9 for c, r in zip(costs, ref["cost"]))          # tie-proof
    assert np.array_equal(state, ref["state"])
    assert np.isfinite(f0).all() and np.array_equal(f0 == 0, state == 0)
    voiced = state > 0
    assert (np.abs(f0 - ref["f0"])[voiced] <= TOL * ref["f0"][voiced]).all()
    assert (state[3] == 0).all()                                            # the row without a candidate


@pytest.mark.parametrize("name", list(TR.e2e_cases()))
def test_end_to_end(name):
    x, kw = TR.e2e_cases()[name]
    ref = TR.track_reference(name)
    f0, state, cp, ca = run_track(x, kw)
    compare_candidates(name, (cp, ca), ref)
    f0, state = f0.cpu().numpy().astype(np.float64), state.cpu().numpy()
    errors = TR.gross_errors(f0, TR.truth(name))
    flips = state != ref["state"]
    same = ~flips & (state > 0)
    e_f0 = (np.abs(f0 - ref["f0"])[same] / ref["f0"][same]).max()
    print(f"{name}: gross errors {errors}; {int(flips.sum())} of {flips.size} states differ; f0 {e_f0:.2e}")
    assert (errors == 0).all()
    assert int(flips.sum()) <= flips.size // 100
    assert e_f0 <= TOL and (f0[~flips & (state == 0)] == 0).all()


@pytest.mark.parametrize("name", TR.PATH_CASES)
def test_tracks_of_the_parity_cases(name):
    x, kw = R.cases()[name]
    ref = TR.track_reference(name)
    assert ref["margin"] >= 1e-6
    f0, state, cp, ca = run_track(x, kw)
    state = state.cpu().numpy()
    flips = state != ref["state"]
    print(f"{name}: {int(flips.sum())} of {flips.size} states differ")
    assert int(flips.sum()) <= flips.size // 100
    # on the kernel's own candidates the path is the reference's path
    own = TR.viterbi(cp.cpu().numpy(), ca.cpu().numpy(), kw["sample_rate"], float(kw["tau_min"]), **TR.COSTS)
    assert own["margin"] >= 1e-6 and np.array_equal(state, own["state"])


def test_strided_rows():
    x, kw = R.cases()["small51"]
    out = run_cand(x, kw, 3, strided=True)
    compare_candidates("strided", out, TR.cand_reference("small51", 3))
    assert all(torch.equal(a, b) for a, b in zip(out, run_cand(x, kw, 3)))
    # the path call takes any strides (it makes its inputs contiguous)
    p, a = run_cand(x, kw, 7)
    wide = torch.full((2,) + tuple(p.shape[:2]) + (9,), float("nan"), device="cuda")
    wide[0, :, :, :7], wide[1, :, :, :7] = p, a
    from golf_amd import functional as GF

    got = GF.f0_viterbi(wide[0, :, :, :7], wide[1, :, :, :7], 8000.0, 4.0, return_state=True)
    want = GF.f0_viterbi(p, a, 8000.0, 4.0, return_state=True)
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_outputs_overwritten_and_null_outputs_untouched():
    """Through the C ABI: outputs pre-filled with NaN (or -1) are written in full, absent slots included; a NULL f0 or state
    is not written and the other comes out the same; the buffer next to an output keeps its fill."""
    from golf_amd import _lib

    lib = _lib.load()
    x, kw = R.cases()["small50"]
    ref = TR.cand_reference("small50", 7)
    B, F, K = ref["period"].shape
    xd = torch.tensor(x).cuda()
    S = kw["W"] + kw["tau_max"]
    buf = torch.full((3, B, F, K), float("nan"), device="cuda")
    rc = lib.golf_f0_candidates_f32(xd.data_ptr(), xd.stride(0), buf[0].data_ptr(), buf[1].data_ptr(), B, x.shape[1], F,
                                    kw["hop"], kw["W"], kw["tau_min"], kw["tau_max"], K, -(S // 2), 0.0, _lib.stream_ptr())
    _lib.check(rc, "golf_f0_candidates_f32")
    assert not torch.isnan(buf[:2]).any() and torch.isnan(buf[2]).all()
    assert ((buf[0] == 0) == (buf[1] == float("inf"))).all() and (buf[0] == 0).any()
    compare_candidates("abi", (buf[0], buf[1]), ref)

    def path(f0, state):
        rc = lib.golf_f0_viterbi_f32(buf[0].data_ptr(), buf[1].data_ptr(), _lib.ptr(f0), _lib.ptr(state), None, 0, B, F, K,
                                     kw["sample_rate"], float(kw["tau_min"]), 0.3, 0.02, 0.35, 0.14, _lib.stream_ptr())
        _lib.check(rc, "golf_f0_viterbi_f32")

    f0 = torch.full((2, B, F), float("nan"), device="cuda")
    state = torch.full((2, B, F), -1, dtype=torch.int32, device="cuda")
    path(f0[0], state[0])
    assert torch.isfinite(f0[0]).all() and torch.isnan(f0[1]).all()
    assert ((state[0] >= 0) & (state[0] <= K)).all() and (state[1] == -1).all() and (state[0] > 0).any()
    f0_only = torch.full((2, B, F), float("nan"), device="cuda")
    path(f0_only[0], None)
    assert torch.equal(f0_only[0], f0[0]) and torch.isnan(f0_only[1]).all()
    state_only = torch.full((2, B, F), -1, dtype=torch.int32, device="cuda")
    path(None, state_only[0])
    assert torch.equal(state_only[0], state[0]) and (state_only[1] == -1).all()


def test_bit_reproducible_and_batch_independent():
    x, kw = R.cases()["recipe"]
    xd = torch.tensor(x).cuda()
    first, second = run_track(xd, kw), run_track(xd, kw)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    for b in (0, 4, 7):
        alone = run_track(xd[b:b + 1], kw)
        assert all(torch.equal(a[0], t[b]) for a, t in zip(alone, first))
    swapped = run_track(xd.flip(0), kw)
    assert all(torch.equal(a.flip(0), t) for a, t in zip(swapped, first))
    # the path through the workspace as well
    _, p, a, _ = TR.path_seed(TR.LDS_FRAMES + 1, 1)
    whole = run_path(p, a)
    assert all(torch.equal(s, t) for s, t in zip(whole, run_path(p, a)))
    assert all(torch.equal(s[0], t[2]) for s, t in zip(run_path(p[2:3], a[2:3]), whole))


def test_graph_capture_replays_the_eager_result():
    x, kw = R.cases()["recipe"]
    xd = torch.tensor(x).cuda()
    eager = run_track(xd, kw)
    static = torch.zeros_like(xd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_track(static, kw)                      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = run_track(static, kw)
    static.copy_(xd)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))


def test_autocast_grad_and_empty_batch():
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError

    x, kw = R.cases()["small50"]
    xd = torch.tensor(x).cuda()
    want = run_track(xd.bfloat16().float(), kw)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = run_track(xd.bfloat16(), kw)
    assert got[0].dtype == got[2].dtype == got[3].dtype == torch.float32 and got[1].dtype == torch.int32
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(GolfError, match="fp32"):
        run_track(xd.bfloat16(), kw)
    with pytest.raises(GolfError, match="fp32"):
        GF.f0_viterbi(want[2].double(), want[3].double(), 8000.0, 4.0)
    out = run_track(xd.clone().requires_grad_(True), kw)
    assert not any(t.requires_grad for t in out) and all(torch.equal(a, b) for a, b in zip(out, run_track(xd, kw)))
    f0 = GF.f0_viterbi(want[2].clone().requires_grad_(True), want[3], 8000.0, 4.0)
    assert isinstance(f0, torch.Tensor) and not f0.requires_grad and torch.equal(f0, want[0])
    F = 777 // 7 + 1
    empty = GF.f0_track(xd[:0], 8000.0, 7, 200.0, 2000.0, 50, return_all=True)
    assert [tuple(t.shape) for t in empty] == [(0, F), (0, F), (0, F, 7), (0, F, 7)] and all(t.is_cuda for t in empty)
    assert empty[1].dtype == torch.int32
    assert GF.f0_track(xd[:0], 8000.0, 7, 200.0, 2000.0, 50, n_candidates=3, n_frames=9).shape == (0, 9)
    assert GF.f0_candidates(xd[:0], 8000.0, 7, 200.0, 2000.0, 50, 2)[1].shape == (0, F, 2)


def test_module():
    from golf_amd import functional as GF
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.f0 import F0Tracker

    x, kw = TR.e2e_cases()["H0.3"]
    xd = torch.tensor(x).cuda()
    m = F0Tracker(R.RECIPE["sr"], R.RECIPE["hop"], window_length=R.RECIPE["W"]).cuda()
    assert (m.tau_min, m.tau_max, m.window_length) == (kw["tau_min"], kw["tau_max"], kw["W"])
    want = GF.f0_track(xd, R.RECIPE["sr"], R.RECIPE["hop"], window_length=R.RECIPE["W"], return_all=True)
    f0 = m(xd)
    assert isinstance(f0, AudioTensor) and f0.hop_length == 240 and f0.shape == (1, 4801 // 240 + 1)
    assert torch.equal(f0.as_tensor(), want[0])
    four = m.analyse(AudioTensor(xd))
    assert len(four) == 4 and all(torch.equal(a, b) for a, b in zip(four, want))
    v = m.voicing(xd)
    assert isinstance(v, AudioTensor) and v.hop_length == 240 and v.as_tensor().dtype == torch.float32
    assert torch.equal(v.as_tensor(), (want[1] > 0).float())
    assert (TR.gross_errors(f0.as_tensor().cpu().numpy(), TR.truth("H0.3")) == 0).all()
    other = F0Tracker(R.RECIPE["sr"], R.RECIPE["hop"], window_length=R.RECIPE["W"], n_candidates=2, unvoiced_cost=0.0).cuda()
    assert other.analyse(xd)[2].shape[-1] == 2 and (other(xd).as_tensor() == 0).all()   # unvoiced costs nothing: never voiced
    with pytest.raises(AssertionError, match="hop 1"):
        m(AudioTensor(xd, 2))
