"""CPU: the host side of the f0 tracker -- the float64 restatement (tests/f0_track_ref.py) against brute force and on the
synthetic signals it is meant for, its fp32 stand-in held to the bars of the GPU test on the GPU test's inputs, the margin that
makes the GPU test's path equality a fair demand, the refusals of the two C entries (none launches), and the module without a
device."""
import math

import numpy as np
import pytest
import torch

import f0_ref as R
import f0_track_ref as TR

TOL = 1e-4


@pytest.mark.parametrize("F,K", [(F, K) for F in (1, 2, 3, 5) for K in (1, 2, 3)])
def test_reference_path_is_the_cheapest_of_all_paths(F, K):
    for seed in range(6):
        p, a = TR.random_candidates(F, K, 1000 + seed)
        for b in range(TR.PATH_B):
            state, f0, cost, margin = TR.viterbi_row(p[b], a[b], 24000.0, 24.0, **TR.COSTS)
            best, argbest = TR.brute_force(p[b], a[b], 24.0, **TR.COSTS)
            assert abs(cost - best) <= 1e-12 and abs(TR.path_cost(state, p[b], a[b], 24.0, **TR.COSTS) - best) <= 1e-12
            if margin > 1e-9:
                assert argbest == [tuple(state)]
            assert ((f0 == 0) == (state == 0)).all()
    # an absent state is never entered: its path costs +inf
    p, a = TR.random_candidates(3, 2, 1)
    assert TR.path_cost([1, 1, 1], p[3], a[3], 24.0, **TR.COSTS) == math.inf


@pytest.mark.parametrize("a1,raw_errors", list(zip(TR.H_A1, (9, 7, 5))))
def test_signal_h_tracked_without_error_where_raw_yin_jumps_octaves(a1, raw_errors):
    name = f"H{a1}"
    x, kw = TR.e2e_cases()[name]
    ref = TR.track_reference(name)
    true = TR.truth(name)
    raw = R.yin(x, threshold=0.3, **kw)
    n_raw, n_low = int(TR.gross_errors(raw["f0"], true)[0]), int(TR.gross_errors(ref["yin"]["f0"], true)[0])
    n_track = int(TR.gross_errors(ref["f0"], true)[0])
    print(f"a1 = {a1}: gross errors raw YIN 0.3: {n_raw}, 0.15: {n_low}, tracked: {n_track}; margin {ref['margin']:.2e}")
    assert n_track == 0
    assert n_raw >= 1 and n_raw == raw_errors


def test_noise_and_gap_rows():
    x, kw = TR.e2e_cases()["noisy"]
    ref = TR.track_reference("noisy")
    true = TR.truth("noisy")
    raw = ref["yin"]   # threshold 0.15
    inner = slice(3, -3)
    print(f"noisy rows: tracked gross errors {TR.gross_errors(ref['f0'], true)}, raw YIN voiced frames "
          f"{raw['voiced'][:, inner].sum(1)}; margin {ref['margin']:.2e}")
    assert (TR.gross_errors(ref["f0"], true) == 0).all()
    assert not raw["voiced"][:, inner].any()
    rec = TR.track_reference("recipe")
    assert (rec["state"][4] == 0).all() and (rec["f0"][4] == 0).all()            # white noise
    assert (rec["state"][5, [10, 11]] == 0).all() and rec["state"][5, 4] > 0 and rec["state"][5, 16] > 0   # the gap
    # the clean tones: 80, 150.3 and 440 Hz stay where raw YIN has them.  The 900 Hz tone (period 26.7 samples, next to
    # tau_min) does not: its double period, 53.3 samples, is sampled closer to its minimum and has the smaller d', and the
    # default lag_cost of 0.02 an octave does not outweigh that -- the path settles an octave low.  Pinned as it is.
    err = [np.abs(rec["f0"][row, 4:-4] / f0 - 1).max() for row, f0 in enumerate(R.RECIPE_TONES)]
    print("tones: worst relative error " + "  ".join(f"{f0} Hz: {e:.2e}" for f0, e in zip(R.RECIPE_TONES, err)))
    assert max(err[:3]) <= 2e-3
    assert np.abs(rec["f0"][3, 4:-4] / 450.0 - 1).max() <= 2e-3


def gpu_inputs():
    """Every case the GPU test runs through the candidate kernel or the whole tracker."""
    return TR.cand_case_names() + ["walk"] + list(TR.e2e_cases())


@pytest.mark.parametrize("name", gpu_inputs())
def test_fp32_stand_in_meets_the_gpu_bars(name):
    x, kw = R.cases()[name] if name in R.cases() else TR.e2e_cases()[name]
    ref = TR.track_reference(name)
    low = TR.candidates(x, fp32=True, **kw)
    low.update(TR.viterbi(low["period"], low["ap"], kw["sample_rate"], float(kw["tau_min"]), **TR.COSTS))
    set_diff = int((ref["lag"] != low["lag"]).any(-1).sum())
    path_diff = int((ref["state"] != low["state"]).sum())
    ok = ref["lag"] >= 0
    e_p = (np.abs(low["period"][ok] - ref["period"][ok]) / ref["period"][ok]).max() if ok.any() else 0.0
    e_ap = np.abs(low["ap"][ok] - ref["ap"][ok]).max() if ok.any() else 0.0
    print(f"{name}: {ref['state'].size} frames, {set_diff} lag sets and {path_diff} states differ; period {e_p:.2e}  "
          f"ap {e_ap:.2e}  margin {ref['margin']:.2e}")
    assert set_diff == 0 and path_diff == 0 and e_p <= TOL and e_ap <= TOL
    assert (low["period"][~ok] == 0).all() and (low["ap"][~ok] == np.inf).all()


@pytest.mark.parametrize("name", list(TR.PATH_CASES) + list(TR.e2e_cases()))
def test_margin_of_the_cases_with_exact_path_equality(name):
    ref = TR.track_reference(name)
    print(f"{name}: margin {ref['margin']:.2e}")
    assert ref["margin"] >= 1e-6


@pytest.mark.parametrize("F,K", TR.PATH_SHAPES + TR.PATH_SHAPES_SWITCH)
def test_margin_of_the_random_candidates(F, K):
    seed, p, a, ref = TR.path_seed(F, K)
    print(f"F = {F}, K = {K}: seed {seed}, margin {ref['margin']:.2e}")
    assert ref["margin"] >= 1e-6
    gone = ~TR.present(p.astype(np.float64), a.astype(np.float64))
    assert gone[3].all() and gone[1, 0].all() and gone[1, -1].all() and gone[2, -1].all()
    if F * K >= 63:
        assert np.isnan(a).any() and ((a == np.inf) & (p > 0)).any() and (gone.all(-1) & ~gone.all((1, 2))[:, None]).any()
        assert (ref["state"] > 0).any() and (ref["state"] == 0).any()


def test_module_and_functional_without_a_device():
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError
    from golf_amd.f0 import F0Analysis, F0Tracker

    assert {"f0_candidates", "f0_viterbi", "f0_track"} <= set(GF.__all__)
    m = F0Tracker(24000, 240)
    assert isinstance(m, F0Analysis) and (m.tau_min, m.tau_max, m.window_length) == (24, 400, 800) and m.n_candidates == 7
    assert (m.unvoiced_cost, m.lag_cost, m.jump_cost, m.switch_cost) == (0.3, 0.02, 0.35, 0.14)
    assert dict(unvoiced_cost=0.3, lag_cost=0.02, jump_cost=0.35, switch_cost=0.14) == GF.F0_VITERBI_COSTS == TR.COSTS
    assert not list(m.parameters()) and not list(m.buffers()) and not m.state_dict()
    x = torch.zeros(1, 1000)
    for call in (m, m.analyse, m.voicing):
        with pytest.raises(GolfError, match="no CPU path"):
            call(x)
    for fn in (GF.f0_candidates, GF.f0_track):
        with pytest.raises(GolfError, match="no CPU path"):
            fn(x, 24000, 240)
        with pytest.raises(GolfError, match="no CPU path"):
            fn(torch.zeros(0, 1000), 24000, 240)
        for kw, what in ((dict(hop=0), "hop"), (dict(f0_max=30000.0), "lags"), (dict(f0_min=2000.0), "f0_min < f0_max"),
                         (dict(window_length=0), "window_length"), (dict(window_length=16000), "exceeds 16384"),
                         (dict(n_frames=0), "n_frames"), (dict(n_frames=2 ** 31), "2\\^31"),
                         (dict(n_candidates=0), "n_candidates"), (dict(n_candidates=8), "n_candidates")):
            with pytest.raises(GolfError, match=what):   # before any tensor is looked at
                fn(x, **dict(dict(sample_rate=24000, hop=240), **kw))
        with pytest.raises(GolfError, match="must be \\(B, T\\)"):
            fn(torch.zeros(1000), 24000, 240)
    p, a = torch.ones(2, 5, 3), torch.zeros(2, 5, 3)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.f0_viterbi(p, a, 24000.0, 24.0)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.f0_viterbi(p[:0], a[:0], 24000.0, 24.0)
    for args, what in (((p[0], a[0], 24000.0, 24.0), "B, F, K"), ((p, a[:, :, :2], 24000.0, 24.0), "B, F, K"),
                       ((torch.ones(2, 5, 8), torch.ones(2, 5, 8), 24000.0, 24.0), "1..7"),
                       ((torch.ones(2, 5, 0), torch.ones(2, 5, 0), 24000.0, 24.0), "1..7"),
                       ((torch.ones(2, 0, 3), torch.ones(2, 0, 3), 24000.0, 24.0), "frames"),
                       ((p, a, 0.0, 24.0), "positive"), ((p, a, 24000.0, 0.0), "positive")):
        with pytest.raises(GolfError, match=what):
            GF.f0_viterbi(*args)


def test_argument_checks_without_gpu():
    """Every refusal comes before a launch, so these calls are safe on a host without a GPU."""
    from golf_amd import _lib

    lib = _lib.load()
    assert "f0_viterbi.hip" in _lib.SOURCES and "f0_yin.hip" in _lib.SOURCES
    assert lib.golf_abi_version() == _lib.ABI_VERSION == 6
    EINVAL, EUNSUPPORTED = -1, -3
    fake = 256   # never dereferenced

    def cand(x=fake, stride=None, period=fake, ap=fake, B=2, T=1000, F=5, hop=240, W=1024, tau_min=24, tau_max=400, K=7):
        return lib.golf_f0_candidates_f32(x, T if stride is None else stride, period, ap, B, T, F, hop, W, tau_min, tau_max, K,
                                          -((W + tau_max) // 2), 0.0, None)

    assert cand(x=None) == EINVAL and b"f0_candidates" in lib.golf_last_error() and b"null" in lib.golf_last_error()
    assert cand(period=None) == EINVAL and cand(ap=None) == EINVAL and b"null" in lib.golf_last_error()
    assert cand(B=0) == EINVAL and cand(F=0) == EINVAL and cand(T=-1) == EINVAL
    assert cand(stride=999) == EINVAL and b"stride" in lib.golf_last_error()
    assert cand(hop=0) == EUNSUPPORTED and b"hop" in lib.golf_last_error()
    assert cand(tau_min=0) == EUNSUPPORTED and cand(tau_max=24) == EUNSUPPORTED and b"exceed tau_min" in lib.golf_last_error()
    assert cand(W=0) == EUNSUPPORTED and b"window" in lib.golf_last_error()
    assert cand(W=16384 - 399) == EUNSUPPORTED and b"LDS" in lib.golf_last_error()
    assert cand(B=1 << 16, F=1 << 15) == EUNSUPPORTED and b"2^31" in lib.golf_last_error()
    assert cand(K=0) == EUNSUPPORTED and b"1..7" in lib.golf_last_error()
    assert cand(K=8) == EUNSUPPORTED and b"f0_candidates" in lib.golf_last_error()

    def path(period=fake, ap=fake, f0=fake, state=fake, ws=None, ws_bytes=0, B=2, F=5, K=7, sr=24000.0, lag_ref=24.0):
        return lib.golf_f0_viterbi_f32(period, ap, f0, state, ws, ws_bytes, B, F, K, sr, lag_ref, 0.3, 0.02, 0.35, 0.14, None)

    assert path(period=None) == EINVAL and b"f0_viterbi" in lib.golf_last_error() and b"null" in lib.golf_last_error()
    assert path(ap=None) == EINVAL
    assert path(f0=None, state=None) == EINVAL and b"at least one output" in lib.golf_last_error()
    assert path(B=0) == EINVAL and path(F=0) == EINVAL and b"bad size" in lib.golf_last_error()
    assert path(sr=0.0) == EINVAL and path(lag_ref=0.0) == EINVAL and b"positive" in lib.golf_last_error()
    assert path(K=0) == EUNSUPPORTED and path(K=8) == EUNSUPPORTED and b"1..7" in lib.golf_last_error()
    assert path(B=1 << 16, F=1 << 15) == EUNSUPPORTED and b"2^31" in lib.golf_last_error()
    # the backpointers of up to 4096 frames live in LDS; beyond that 8 bytes a frame in the workspace
    ws = lib.golf_f0_viterbi_workspace_bytes
    assert TR.LDS_FRAMES == 4096
    assert ws(5, 1, 7) == ws(5, 4096, 1) == ws(1 << 18, 4096, 7) == 0
    assert ws(5, 4097, 1) == 5 * 4097 * 8 and ws(1, 4097, 7) == 4097 * 8 and ws(3, 1 << 20, 2) == 3 * (1 << 20) * 8
    assert ws(0, 5000, 7) == ws(5, 0, 7) == ws(5, 5000, 0) == ws(5, 5000, 8) == 0
    assert path(F=4097) == EINVAL and b"workspace" in lib.golf_last_error()                       # needed and NULL
    assert path(F=4097, ws=fake, ws_bytes=2 * 4097 * 8 - 1) == EINVAL and b"workspace" in lib.golf_last_error()
