"""GPU: the streaming analysis -- the fixed-lag path kernel (golf_f0_viterbi_stream_f32, functional.f0_viterbi_stream) against
the float64 restatement of its definition (tests/f0_stream_ref.py, pinned by tests/test_f0_stream_host.py) and against itself
under every cut, the hygiene of its carry, and the three streams of golf_amd/analysis_stream.py against their one-shot modules.

Bars.  Path: the states equal the reference's exactly (the host test asserts a margin >= 1e-6 for every shape and lag; the
kernel's float64 costs differ from the reference's by roundoff), f0 within 1e-4 relative on voiced frames and exactly 0 in
state 0; every cut gives the same bits, and a lag of the whole utterance gives ``functional.f0_viterbi``'s bits.  Streams:
``torch.equal`` to the one-shot module, whatever the cuts."""
import numpy as np
import pytest
import torch

import f0_ref as R
import f0_stream_ref as SR
import f0_track_ref as TR

pytestmark = pytest.mark.gpu

TOL = 1e-4
SR_, REF = 24000.0, 24.0


# ---- the path kernel alone ----------------------------------------------------------------------------------------------------
def stream_path(pd, ad, lag, cuts, alone=False, carry=None):
    """Device candidates (B, F, K) through the cuts -> (f0, state) on the device, concatenated."""
    from golf_amd import functional as GF

    B, F, K = pd.shape
    if carry is None:
        carry = GF.f0_viterbi_stream_state(B, K, lag, pd.device)
    f0s, states = [], []
    for f_done, nf, flush, first, n_out in SR.calls(cuts, lag, alone):
        f0, state = GF.f0_viterbi_stream(pd[:, f_done:f_done + nf], ad[:, f_done:f_done + nf], carry, f_done, lag, SR_, REF,
                                         flush=flush, return_state=True, **TR.COSTS)
        assert f0.shape == state.shape == (B, n_out) and f0.dtype == torch.float32 and state.dtype == torch.int32
        assert not f0.requires_grad
        f0s.append(f0), states.append(state)
    return torch.cat(f0s, 1), torch.cat(states, 1)


def candidates(F, K):
    seed, p, a, refs = SR.path_seed(F, K)
    return torch.tensor(p).cuda(), torch.tensor(a).cuda(), refs


@pytest.mark.parametrize("F,K", SR.PATH_SHAPES)
def test_path_kernel_alone(F, K):
    from golf_amd import functional as GF

    pd, ad, refs = candidates(F, K)
    one_shot = GF.f0_viterbi(pd, ad, SR_, REF, return_state=True, **TR.COSTS)
    for lag in SR.lags_of(F):
        ref = refs[lag]
        assert ref["margin"] >= 1e-6
        outs = {name: stream_path(pd, ad, lag, cuts, alone) for name, (cuts, alone) in SR.cut_lists(F, lag).items()}
        f0d, stated = outs["one"]
        assert f0d.shape == stated.shape == (TR.PATH_B, F)
        f0, state = f0d.cpu().numpy().astype(np.float64), stated.cpu().numpy()
        voiced = state > 0
        e_f0 = (np.abs(f0 - ref["f0"])[voiced] / ref["f0"][voiced]).max() if voiced.any() else 0.0
        print(f"F = {F}, K = {K}, lag {lag}: {int((state != ref['state']).sum())} states differ; f0 {e_f0:.2e}")
        assert np.array_equal(state, ref["state"])
        assert np.isfinite(f0).all() and np.array_equal(f0 == 0, state == 0) and e_f0 <= TOL
        assert (state[3] == 0).all() and (f0[3] == 0).all()                 # the row without a candidate
        for name, (f0c, statec) in outs.items():
            assert torch.equal(f0c, f0d) and torch.equal(statec, stated), (lag, name)
        if lag >= F - 1:
            assert torch.equal(f0d, one_shot[0]) and torch.equal(stated, one_shot[1])


def test_a_frame_per_call_wraps_the_ring():
    """(400, 2), a frame per call at lag 65: every ring slot of the carry is reused six times."""
    pd, ad, refs = candidates(400, 2)
    f0, state = stream_path(pd, ad, 65, [1] * 400)
    assert np.array_equal(state.cpu().numpy(), refs[65]["state"])
    whole = stream_path(pd, ad, 65, [400])
    assert torch.equal(f0, whole[0]) and torch.equal(state, whole[1])
    assert (state.cpu().numpy() != refs[399]["state"]).sum() == (refs[65]["state"] != refs[399]["state"]).sum()


@pytest.mark.parametrize("F,K", [(1057, 1), (1057, 7), (2113, 1)])
def test_one_call_longer_than_a_chunk(F, K):
    """One call of more than 1024 frames: the kernel decides between its chunks, and past 2048 frames its LDS rings wrap
    inside the call.  1057 = 1024 + 33 ends on a block of one frame; 2113 = 2048 + 65.  Seed 0, lags 8 and 1024 (the kernel
    takes no more), the reference for these two alone."""
    p, a = TR.random_candidates(F, K, 0)
    pd, ad = torch.tensor(p).cuda(), torch.tensor(a).cuda()
    within = [500, 524] + [1024] * ((F - 1024) // 1024) + [(F - 1024) % 1024]   # no call crosses a chunk
    assert sum(within) == F and max(within) <= 1024
    for lag in (8, 1024):
        ref = SR.fixed_lag(p, a, lag, SR_, REF, **TR.COSTS)
        assert ref["margin"] >= 1e-6
        f0d, stated = stream_path(pd, ad, lag, [F])
        f0, state = f0d.cpu().numpy().astype(np.float64), stated.cpu().numpy()
        voiced = state > 0
        e_f0 = (np.abs(f0 - ref["f0"])[voiced] / ref["f0"][voiced]).max() if voiced.any() else 0.0
        print(f"F = {F}, K = {K}, lag {lag}: margin {ref['margin']:.1e}; {int((state != ref['state']).sum())} states differ; "
              f"f0 {e_f0:.2e}")
        assert np.array_equal(state, ref["state"])
        assert np.isfinite(f0).all() and np.array_equal(f0 == 0, state == 0) and e_f0 <= TOL
        for cuts, alone in ((within, False), ([F], True)):
            f0c, statec = stream_path(pd, ad, lag, cuts, alone)
            assert torch.equal(f0c, f0d) and torch.equal(statec, stated), (lag, cuts, alone)


# ---- the carry ----------------------------------------------------------------------------------------------------------------
CARRY_SHAPE, CARRY_LAG = (130, 7), 7


def test_carry_prefilled_and_canary():
    from golf_amd import _lib

    pd, ad, refs = candidates(*CARRY_SHAPE)
    B, F, K = pd.shape
    words = _lib.load().golf_f0_viterbi_stream_state_bytes(B, K, CARRY_LAG) // 8
    cuts, alone = SR.cut_lists(F, CARRY_LAG)["random"]
    want = stream_path(pd, ad, CARRY_LAG, cuts, alone, torch.zeros(words, dtype=torch.int64, device="cuda"))
    assert np.array_equal(want[1].cpu().numpy(), refs[CARRY_LAG]["state"])
    canary = 0x5A5A5A5A5A5A5A5A
    big = torch.full((words + 64,), -1, dtype=torch.int64, device="cuda")   # 0xFF bytes
    big[words:] = canary
    got = stream_path(pd, ad, CARRY_LAG, cuts, alone, big)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert (big[words:] == canary).all()
    again = stream_path(pd, ad, CARRY_LAG, [F], False, big)                 # a carry left by another utterance
    assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])


def test_two_utterances_interleaved_on_two_carries():
    from golf_amd import functional as GF

    F, K = CARRY_SHAPE
    lag = CARRY_LAG
    pa, aa, _ = candidates(F, K)
    p2, a2 = TR.random_candidates(F, K, 77)
    pb, ab = torch.tensor(p2).cuda(), torch.tensor(a2).cuda()
    alone_a, alone_b = stream_path(pa, aa, lag, [F]), stream_path(pb, ab, lag, [F])
    carries = [GF.f0_viterbi_stream_state(TR.PATH_B, K, lag, "cuda") for _ in range(2)]
    outs = ([], [])
    calls_a, calls_b = SR.calls([5] * (F // 5), lag), SR.calls([13] * (F // 13), lag)
    for i in range(max(len(calls_a), len(calls_b))):
        for which, (p, a, calls) in enumerate(((pa, aa, calls_a), (pb, ab, calls_b))):
            if i < len(calls):
                f_done, nf, flush, first, n_out = calls[i]
                outs[which].append(GF.f0_viterbi_stream(p[:, f_done:f_done + nf], a[:, f_done:f_done + nf], carries[which],
                                                        f_done, lag, SR_, REF, flush=flush, return_state=True, **TR.COSTS))
    for out, alone in zip(outs, (alone_a, alone_b)):
        assert torch.equal(torch.cat([o[0] for o in out], 1), alone[0])
        assert torch.equal(torch.cat([o[1] for o in out], 1), alone[1])


def test_bit_reproducible_and_batch_independent():
    pd, ad, _ = candidates(*CARRY_SHAPE)
    F = pd.shape[1]
    cuts, alone = SR.cut_lists(F, CARRY_LAG)["random"]
    first, second = stream_path(pd, ad, CARRY_LAG, cuts, alone), stream_path(pd, ad, CARRY_LAG, cuts, alone)
    assert all(torch.equal(s, t) for s, t in zip(first, second))
    for b in (0, 2, 4):
        row = stream_path(pd[b:b + 1], ad[b:b + 1], CARRY_LAG, cuts, alone)
        assert all(torch.equal(s[0], t[b]) for s, t in zip(row, first))
    flipped = stream_path(pd.flip(0), ad.flip(0), CARRY_LAG, cuts, alone)
    assert all(torch.equal(s.flip(0), t) for s, t in zip(flipped, first))


def test_null_outputs_untouched_and_strided_output():
    """Through the C ABI: a NULL f0 or state is not written and the other comes out the same; an output with a row stride
    beyond n_out keeps the fill of its gap."""
    from golf_amd import _lib

    lib = _lib.load()
    pd, ad, refs = candidates(*CARRY_SHAPE)
    B, F, K = pd.shape
    lag = CARRY_LAG
    nbytes = lib.golf_f0_viterbi_stream_state_bytes(B, K, lag)

    def run(want_f0, want_state, gap):
        carry = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
        f0 = torch.full((B, F + gap), float("nan"), device="cuda")
        state = torch.full((B, F + gap), -1, dtype=torch.int32, device="cuda")
        at = 0
        for f_done, nf, flush, first, n_out in SR.calls([50, 3, 77], lag):
            p, a = pd[:, f_done:f_done + nf].contiguous(), ad[:, f_done:f_done + nf].contiguous()
            rc = lib.golf_f0_viterbi_stream_f32(p.data_ptr(), a.data_ptr(), f0[:, at:].data_ptr() if want_f0 else None,
                                                state[:, at:].data_ptr() if want_state else None, F + gap, carry.data_ptr(),
                                                nbytes, B, nf, K, lag, f_done, int(flush), SR_, REF, 0.3, 0.02, 0.35, 0.14,
                                                _lib.stream_ptr())
            _lib.check(rc, "golf_f0_viterbi_stream_f32")
            at += n_out
        assert at == F
        return f0, state

    f0, state = run(True, True, 0)
    assert np.array_equal(state.cpu().numpy(), refs[lag]["state"]) and torch.isfinite(f0).all()
    f0_only, untouched = run(True, False, 0)
    assert torch.equal(f0_only, f0) and (untouched == -1).all()
    untouched, state_only = run(False, True, 0)
    assert torch.equal(state_only, state) and torch.isnan(untouched).all()
    f0_wide, state_wide = run(True, True, 5)
    assert torch.equal(f0_wide[:, :F], f0) and torch.equal(state_wide[:, :F], state)
    assert torch.isnan(f0_wide[:, F:]).all() and (state_wide[:, F:] == -1).all()


def test_functional_checks_on_the_device():
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError

    pd, ad, _ = candidates(65, 1)
    carry = GF.f0_viterbi_stream_state(TR.PATH_B, 1, 4, "cuda")
    nothing = GF.f0_viterbi_stream(pd[:, :0], ad[:, :0], carry, 0, 4, SR_, REF, return_state=True)   # launches nothing
    assert [tuple(t.shape) for t in nothing] == [(TR.PATH_B, 0)] * 2 and nothing[1].dtype == torch.int32
    assert GF.f0_viterbi_stream(pd[:, :3], ad[:, :3], carry, 0, 4, SR_, REF).shape == (TR.PATH_B, 0)
    with pytest.raises(GolfError, match="fp32"):
        GF.f0_viterbi_stream(pd.double(), ad.double(), carry, 0, 4, SR_, REF)
    with pytest.raises(GolfError, match="carry"):
        GF.f0_viterbi_stream(pd, ad, carry[:-1], 0, 4, SR_, REF)
    want = GF.f0_viterbi_stream(pd.bfloat16().float(), ad.bfloat16().float(), carry, 0, 4, SR_, REF, flush=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = GF.f0_viterbi_stream(pd.bfloat16(), ad.bfloat16(), carry, 0, 4, SR_, REF, flush=True)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    out = GF.f0_viterbi_stream(pd.clone().requires_grad_(True), ad, carry, 0, 4, SR_, REF, flush=True)
    assert not out.requires_grad


# ---- the streams ----------------------------------------------------------------------------------------------------------------
F0_CASES = ("recipe", "edges", "small50", "small51", "from0", "hop_gt_W", "S_gt_T")
# (B, T, W, hop, M): the smallest cases of tests/test_gpu_lpc_analysis.py, each with both values of centred
LPC_CASES = {"odd50": (5, 777, 50, 7, 13), "odd51": (5, 777, 51, 7, 13), "hop>W": (1, 300, 128, 200, 8), "W>T": (2, 100, 256, 64, 4)}


def wave_cuts(T, hop, span, seed):
    """name -> block lengths: one push, pushes of hop, pushes of one sample (the 777-sample cases only), a seeded random cut
    with empty blocks and blocks longer than a frame, and nothing pushed at all (an utterance of no samples)."""
    rng = np.random.default_rng(seed)
    rand, left = [0], T
    while left:
        r = rng.random()
        n = 0 if r < 0.15 else int(rng.integers(span + 1, 2 * span + hop + 2)) if r < 0.4 else int(rng.integers(1, hop + 3))
        n = min(n, left)
        rand.append(n)
        left -= n
    assert 0 in rand and (max(rand) > span or T <= span)
    cuts = {"one": [T], "hop": [hop] * (T // hop) + ([T % hop] if T % hop else []), "random": rand + [0]}
    if T == 777:
        cuts["sample"] = [1] * T
    return cuts


def freqs(kw):
    """The frequencies that give the explicit lags of a case."""
    from golf_amd import functional as GF

    sr = kw["sample_rate"]
    f0_max, f0_min = sr / (kw["tau_min"] + 0.5), sr / (kw["tau_max"] - 0.5)
    assert GF.f0_lags(sr, f0_min, f0_max, kw["W"]) == (kw["tau_min"], kw["tau_max"], kw["W"])
    return f0_min, f0_max


def f0_module(cls, kw, **more):
    f0_min, f0_max = freqs(kw)
    return cls(kw["sample_rate"], kw["hop"], f0_min, f0_max, kw["W"], kw.get("threshold", 0.15), kw.get("rms_floor", 0.0),
               kw.get("centred", True), **more).cuda()


def pushed(stream, x, cuts, method="push_all"):
    """Everything the stream gives for x cut into the blocks, plus finish: lists of per-call results."""
    push, finish = (stream.push_all, stream.finish_all) if method == "push_all" else (stream.push, stream.finish)
    out, at = [], 0
    for n in cuts:
        out.append(push(x[:, at:at + n]))
        at += n
    assert at == x.shape[1]
    out.append(finish())
    return out


def joined(parts):
    """Per-call tuples of tensors -> the tuple of their concatenations along the frame axis."""
    return tuple(torch.cat([p[i] for p in parts], 1) for i in range(len(parts[0])))


@pytest.mark.parametrize("name", F0_CASES)
def test_f0_stream_equals_the_module(name):
    from golf_amd.analysis_stream import F0Stream
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.f0 import F0Analysis

    x, kw = R.cases()[name]
    xd = torch.tensor(x).cuda()
    m = f0_module(F0Analysis, kw)
    want = m.analyse(xd)
    stream = F0Stream(m, xd.shape[0])
    S = kw["W"] + kw["tau_max"]
    for cut, blocks in wave_cuts(xd.shape[1], kw["hop"], S, 3).items():   # the same stream: finish() resets it
        parts = pushed(stream, xd, blocks)
        got = joined(parts)
        assert all(g.dtype == w.dtype and torch.equal(g, w) for g, w in zip(got, want)), (name, cut)
        assert len(got) == 3 and stream.pushed == 0 and stream.framed == 0
    parts = pushed(stream, AudioTensor(xd), wave_cuts(xd.shape[1], kw["hop"], S, 4)["random"], "push")
    assert all(isinstance(p, AudioTensor) and p.hop_length == kw["hop"] for p in parts)
    assert any(p.shape[1] == 0 for p in parts)
    assert torch.equal(torch.cat([p.as_tensor() for p in parts], 1), m(xd).as_tensor())
    with_v = F0Stream(m, xd.shape[0], voicing=True)
    parts = pushed(with_v, xd, [xd.shape[1]], "push")
    assert all(isinstance(t, AudioTensor) and t.hop_length == kw["hop"] for p in parts for t in p)
    assert torch.equal(torch.cat([p[1].as_tensor() for p in parts], 1), m.voicing(xd).as_tensor())
    # nothing pushed at all: the utterance of no samples
    nothing = stream.finish_all()
    assert all(torch.equal(g, w) for g, w in zip(nothing, m.analyse(xd[:, :0])))


@pytest.mark.parametrize("name", F0_CASES)
def test_tracker_stream_equals_the_definition_and_the_module(name):
    from golf_amd import functional as GF
    from golf_amd.analysis_stream import F0TrackerStream, open_analysis_stream
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.f0 import F0Tracker

    x, kw = R.cases()[name]
    xd = torch.tensor(x).cuda()
    B, T = xd.shape
    m = f0_module(F0Tracker, kw)
    f0_full, state_full, cp, ca = m.analyse(xd)
    F = f0_full.shape[1]
    S = kw["W"] + kw["tau_max"]
    for lag in (2, 8, max(F - 1, 0), 1024):
        stream = open_analysis_stream(m, B, lag=lag)
        assert isinstance(stream, F0TrackerStream) and stream.lag == lag
        carry = GF.f0_viterbi_stream_state(B, 7, lag, "cuda")
        want = GF.f0_viterbi_stream(cp, ca, carry, 0, lag, kw["sample_rate"], float(kw["tau_min"]), flush=True, return_state=True)
        if lag >= F - 1:
            assert torch.equal(want[0], f0_full) and torch.equal(want[1], state_full)
        for cut, blocks in wave_cuts(T, kw["hop"], S, 5).items():
            if cut == "sample" and lag not in (2, 1024):
                continue
            got = joined(pushed(stream, xd, blocks))
            assert got[1].dtype == torch.int32 and got[0].dtype == torch.float32
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (name, lag, cut)
            assert stream.pushed == 0 and stream.framed == 0
    stream = F0TrackerStream(m, B, lag=1024, voicing=True)
    parts = pushed(stream, AudioTensor(xd), wave_cuts(T, kw["hop"], S, 6)["random"], "push")
    assert all(isinstance(t, AudioTensor) and t.hop_length == kw["hop"] for p in parts for t in p)
    assert torch.equal(torch.cat([p[0].as_tensor() for p in parts], 1), m(xd).as_tensor())
    assert torch.equal(torch.cat([p[1].as_tensor() for p in parts], 1), m.voicing(xd).as_tensor())
    nothing = F0TrackerStream(m, B).finish_all()
    empty = m.analyse(xd[:, :0])
    assert torch.equal(nothing[0], empty[0]) and torch.equal(nothing[1], empty[1])


@pytest.mark.parametrize("name", list(TR.e2e_cases()))
def test_tracker_stream_at_the_default_lag_end_to_end(name):
    from golf_amd.analysis_stream import F0TrackerStream
    from golf_amd.f0 import F0Tracker

    x, kw = TR.e2e_cases()[name]
    xd = torch.tensor(x).cuda()
    m = f0_module(F0Tracker, kw)
    stream = F0TrackerStream(m, xd.shape[0])
    assert stream.lag == SR.DEFAULT_LAG == 8
    f0, state = joined(pushed(stream, xd, wave_cuts(xd.shape[1], kw["hop"], kw["W"] + kw["tau_max"], 7)["hop"]))
    one_shot = m.analyse(xd)
    errors = TR.gross_errors(f0.cpu().numpy(), TR.truth(name))
    flips = int((state != one_shot[1]).sum())
    print(f"{name}: gross errors {errors}; {flips} of {state.numel()} states differ from the one-shot path")
    assert (errors == 0).all()
    assert flips <= state.numel() // 100


@pytest.mark.parametrize("centred", (True, False))
@pytest.mark.parametrize("name", list(LPC_CASES))
def test_lpc_stream_equals_the_module(name, centred):
    from golf_amd.analysis_stream import LPCAnalysisStream
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.lpc import LPCAnalysis

    B, T, W, hop, M = LPC_CASES[name]
    xd = torch.tensor(np.random.default_rng(sum(map(ord, name))).normal(0, 1, (B, T)).astype(np.float32)).cuda()
    m = LPCAnalysis(M, hop, W, centred=centred).cuda()
    want = m.analyse(xd, return_rc=True)
    stream = LPCAnalysisStream(m, B, return_rc=True)
    for cut, blocks in wave_cuts(T, hop, W, 8).items():
        got = joined(pushed(stream, xd, blocks))
        assert len(got) == 3 and all(g.dtype == w.dtype and torch.equal(g, w) for g, w in zip(got, want)), (name, cut)
        assert stream.pushed == 0 and stream.framed == 0
    plain = LPCAnalysisStream(m, B)
    parts = pushed(plain, AudioTensor(xd), wave_cuts(T, hop, W, 9)["random"], "push")
    assert all(len(p) == 2 and all(isinstance(t, AudioTensor) and t.hop_length == hop for t in p) for p in parts)
    gain, a = m(xd)
    assert torch.equal(torch.cat([p[0].as_tensor() for p in parts], 1), gain.as_tensor())
    assert torch.equal(torch.cat([p[1].as_tensor() for p in parts], 1), a.as_tensor())
    nothing = stream.finish_all()
    assert all(torch.equal(g, w) for g, w in zip(nothing, m.analyse(xd[:, :0], return_rc=True)))


def test_streams_refuse_by_name():
    from golf_amd.analysis_stream import F0Stream, F0TrackerStream, LPCAnalysisStream
    from golf_amd._lib import GolfError
    from golf_amd.f0 import F0Analysis, F0Tracker
    from golf_amd.lpc import LPCAnalysis

    x, kw = R.cases()["small50"]
    xd = torch.tensor(x).cuda()
    B = xd.shape[0]
    streams = (F0Stream(f0_module(F0Analysis, kw), B), F0TrackerStream(f0_module(F0Tracker, kw), B),
               LPCAnalysisStream(LPCAnalysis(13, 7, 50).cuda(), B))
    for s in streams:
        with pytest.raises(NotImplementedError, match="requires grad"):
            s.push(xd.clone().requires_grad_(True))
        with pytest.raises(GolfError, match="fp32"):
            s.push(xd.half())
        with pytest.raises(ValueError, match=f"B={B}"):
            s.push(xd[:2])
        assert s.pushed == 0                                   # a refused block leaves the stream as it was
        want = joined(pushed(type(s)(s.module, B), xd.half().float(), [300, 477]))
        with torch.autocast("cuda", dtype=torch.float16):
            got = joined(pushed(s, xd.half(), [300, 477]))
        assert all(g.dtype == w.dtype and torch.equal(g, w) for g, w in zip(got, want))
        with torch.no_grad():                                  # a leaf that requires grad is fine where no graph is built
            s.push(xd.clone().requires_grad_(True))
            s.finish()
