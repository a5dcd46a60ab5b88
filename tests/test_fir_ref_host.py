"""The yardsticks of tests/test_gpu_fir_family.py, checked on the CPU (tests/fir_ref.py): each float64 reference against
an independent float64 computation (torch conv1d / unfold under autograd, and the oracle where it overlaps), the adjoint
identities, that the GPU tests' exact inputs tell a subtly wrong kernel from a right one by >= 100 bars, and that a
sequential float32 sum of every GPU case stays within a third of its bar."""
import functools

import numpy as np
import pytest
import torch

import fir_ref as R
from conftest import rel_err

F64 = torch.float64
LTI_ALL = R.LTI_CASES + [R.LTI_LARGEST, R.LTI_BATCH]
FRAME_IDS = [(cid, causal) for cid in R.FRAMES_CASES for causal in (False, True)]


def agree(got, want, what, tol=1e-12):
    emax, el2 = rel_err(got, want)
    print(f"{what}: rel-max {emax:.3e} rel-l2 {el2:.3e}")
    assert emax <= tol and el2 <= tol, (what, emax, el2)


def differ(wrong, right, what, bar):
    """A wrong reference must miss the right one by >= 100 bars.  The GPU check fails as soon as EITHER norm passes the
    bar, so the margin is the larger of the two: a mistake confined to a few taps (the ragged tail at lead 0 touches two) is
    large in the max norm and small in L2."""
    emax, el2 = rel_err(wrong, right)
    print(f"{what}: wrong reference is off by rel-max {emax:.3e} rel-l2 {el2:.3e} (bar {bar:g})")
    assert max(emax, el2) >= 100 * bar, (what, emax, el2)


def within_third(got, want, what, bar):
    emax, el2 = rel_err(got, want)
    print(f"{what}: sequential fp32 rel-max {emax:.3e} rel-l2 {el2:.3e} (bar/3 {bar / 3:.2e})")
    assert max(emax, el2) <= bar / 3, (what, emax, el2)


# ------------------------------------------------------------------------------------------------ cached references
@functools.lru_cache(maxsize=None)
def lti_ref(case):
    ex, taps, gy = R.lti_inputs(*case)
    lead = case[3]
    return (R.lti_fir(ex, taps, lead),) + R.lti_fir_grads(gy, ex, taps, lead)


@functools.lru_cache(maxsize=None)
def frames_ref(cid, causal):
    c = R.frames_inputs(cid, causal)
    y = R.frames_fir(c["ex"], c["kern"], c["hop"], causal, c["frame0"])
    return (y,) + R.frames_fir_grads(c["gy"], c["ex"], c["kern"], c["hop"], causal, c["frame0"])


@functools.lru_cache(maxsize=None)
def decim_ref(case):
    os_, K, N = case
    x, taps, g = R.decim_inputs(*case)
    return R.decimate(x, taps, os_), R.decimate_adjoint(g, taps, os_, N)


# ------------------------------------------------------------------------------------------------ independent float64
def torch_lti(ex, taps, lead, gy):
    x, t = torch.tensor(ex, dtype=F64, requires_grad=True), torch.tensor(taps, dtype=F64, requires_grad=True)
    K = t.numel()
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (lead, K - 1 - lead))[:, None], t[None, None])[:, 0]
    gx, gt = torch.autograd.grad(y, (x, t), torch.tensor(gy, dtype=F64))
    return y.detach().numpy(), gx.numpy(), gt.numpy()


def torch_frames(c):
    """unfold twice: frames of N+hop-1 samples every hop, windows of N inside a frame."""
    N, hop, nfr, f0, causal = c["N"], c["hop"], c["nfr"], c["frame0"], c["causal"]
    x = torch.tensor(c["ex"], dtype=F64, requires_grad=True)
    k = torch.tensor(c["kern"], dtype=F64, requires_grad=True)
    P = N - 1 if causal else (N - 1) // 2
    xp = torch.nn.functional.pad(x, (P, N))
    fr = xp.unfold(1, N + hop - 1, hop)[:, :nfr].unfold(2, N, 1)          # (B, nfr, hop, N)
    rows = k[:, f0: f0 + nfr]
    rows = rows.flip(-1) if causal else rows
    y = (fr * rows[:, :, None, :]).sum(-1).reshape(x.shape[0], nfr * hop)
    gx, gk = torch.autograd.grad(y, (x, k), torch.tensor(c["gy"], dtype=F64))
    return y.detach().numpy(), gx.numpy(), gk.numpy()


def torch_decimate(x, taps, os_, g):
    xt = torch.tensor(x, dtype=F64, requires_grad=True)
    t = torch.tensor(taps, dtype=F64)
    y = torch.nn.functional.conv1d(xt[:, None], t[None, None], stride=os_, padding=(t.numel() - 1) // 2)[:, 0]
    (gx,) = torch.autograd.grad(y, xt, torch.tensor(g, dtype=F64))
    return y.detach().numpy(), gx.numpy()


@pytest.mark.parametrize("case", LTI_ALL, ids=str)
def test_lti_reference_vs_torch(case):
    ex, taps, gy = R.lti_inputs(*case)
    for name, got, want in zip(("y", "g_ex", "g_taps"), lti_ref(case), torch_lti(ex, taps, case[3], gy)):
        agree(got, want, f"lti {case} {name}")


@pytest.mark.parametrize("K,T", [(7, 100), (11, 5), (251, 300)])
def test_lti_reference_vs_oracle_room_filter(K, T):
    """LTIAcousticFilter is the LTI FIR with taps [kernel, 1] and lead = K."""
    from oracle import golf_oracle as O

    rng = np.random.default_rng(K)
    ex, kernel, gy = rng.normal(0, 1, (2, T)), rng.normal(0, 1, K), rng.normal(0, 1, (2, T))
    taps = np.concatenate([kernel, [1.0]])
    agree(R.lti_fir(ex, taps, K), O.lti_acoustic_filter_forward(ex, kernel), "room fwd")
    g_ex, g_taps = R.lti_fir_grads(gy, ex, taps, K)
    o_ex, o_k = O.lti_acoustic_filter_backward(gy, ex, kernel)
    agree(g_ex, o_ex, "room g_ex")
    agree(g_taps[:K], o_k, "room g_kernel")


@pytest.mark.parametrize("cid,causal", FRAME_IDS)
def test_frames_reference_vs_torch(cid, causal):
    c = R.frames_inputs(cid, causal)
    for name, got, want in zip(("y", "g_ex", "g_kern"), frames_ref(cid, causal), torch_frames(c)):
        agree(got, want, f"frames {cid} causal={causal} {name}")


@pytest.mark.parametrize("cid", ["mod4-N50", "tile-hop252", "many-frames", "unused-rows", "odd-hop7"])
def test_frames_reference_vs_oracle(cid):
    from oracle import golf_oracle as O
    import minphase_ref

    c = R.frames_inputs(cid, False)
    agree(frames_ref(cid, False)[0], O.ltv_fir_frames_forward(c["ex"], c["kern"], c["hop"]), f"{cid} vs oracle")
    c = R.frames_inputs(cid, True)
    want = minphase_ref.causal_frames(torch.tensor(c["ex"], dtype=F64), torch.tensor(c["kern"], dtype=F64), c["hop"])
    agree(frames_ref(cid, True)[0], want.numpy(), f"{cid} vs minphase_ref.causal_frames")


@pytest.mark.parametrize("case", R.DECIM_CASES + R.DECIM_ADJ_CASES, ids=str)
def test_decimator_reference_vs_torch_and_oracle(case):
    from oracle import golf_oracle as O

    os_, K, N = case
    x, taps, g = R.decim_inputs(*case)
    y, gx = decim_ref(case)
    ty, tgx = torch_decimate(x, taps, os_, g)
    agree(y, ty, f"decimate {case}")
    agree(gx, tgx, f"decimate adjoint {case}")
    agree(y, O.decimate_fir(x, taps, os_), f"decimate {case} vs oracle")
    agree(gx, O.decimate_fir_adjoint(g, taps, os_, N), f"decimate adjoint {case} vs oracle")


def test_designed_taps_are_what_the_cases_say():
    assert [R.decimator_taps(os_).shape[0] for os_ in (2, 3, 4)] == [65, 97, 129]


# ------------------------------------------------------------------------------------------------ adjoint identities
def _dot_agree(a, b, c, d, what, tol=1e-12):
    """<a,b> = <c,d> to ``tol`` of the sum of the products' magnitudes (what a float64 dot product is accurate to)."""
    a, b, c, d = (np.asarray(v, np.float64) for v in (a, b, c, d))
    lhs, rhs = (a * b).sum(), (c * d).sum()
    scale = max(np.abs(a * b).sum(), np.abs(c * d).sum(), 1e-300)
    print(f"{what}: <Ax,g> {lhs:.15e} <x,A'g> {rhs:.15e} (|difference| / scale {abs(lhs - rhs) / scale:.2e})")
    assert abs(lhs - rhs) <= tol * scale, (what, lhs, rhs)


@pytest.mark.parametrize("case", R.LTI_CASES, ids=str)
def test_lti_adjoint_identity(case):
    ex, taps, gy = (v.astype(np.float64) for v in R.lti_inputs(*case))
    y, g_ex, g_taps = lti_ref(case)
    _dot_agree(y, gy, ex, g_ex, f"lti {case} in ex")
    _dot_agree(y, gy, taps, g_taps, f"lti {case} in taps")          # bilinear: linear in the taps too


@pytest.mark.parametrize("cid,causal", FRAME_IDS)
def test_frames_adjoint_identity(cid, causal):
    c = R.frames_inputs(cid, causal)
    y, g_ex, g_kern = frames_ref(cid, causal)
    _dot_agree(y, c["gy"], c["ex"], g_ex, f"frames {cid} in ex")
    _dot_agree(y, c["gy"], c["kern"], g_kern, f"frames {cid} in kern")


@pytest.mark.parametrize("case", R.DECIM_ADJ_CASES, ids=str)
def test_decimator_adjoint_identity(case):
    x, taps, g = R.decim_inputs(*case)
    y, gx = decim_ref(case)
    _dot_agree(y, g, x, gx, f"decimate {case}")


# ------------------------------------------------------------------------------------------------ discrimination
@pytest.mark.parametrize("case", LTI_ALL, ids=str)
def test_lti_inputs_see_wrong_kernels(case):
    B, T, K, lead = case
    ex, taps, gy = R.lti_inputs(*case)
    y, g_ex, g_taps = lti_ref(case)
    mirrored = taps[::-1]
    differ(R.lti_fir(ex, mirrored, lead), y, "taps mirrored: y", R.FWD_BAR)
    differ(R.lti_fir_grads(gy, ex, mirrored, lead)[0], g_ex, "taps mirrored: g_ex", R.GRAD_BAR)
    differ(R.lti_fir_grads(gy, ex, taps, lead)[1][::-1], g_taps, "taps mirrored: g_taps", R.GRAD_BAR)
    short = taps.copy()
    short[-1] = 0
    if K - 1 - lead < T:                                 # the last tap reaches a sample at all
        differ(R.lti_fir(ex, short, lead), y, "last tap dropped: y", R.FWD_BAR)
        differ(R.lti_fir_grads(gy, ex, short, lead)[0], g_ex, "last tap dropped: g_ex", R.GRAD_BAR)
        dropped = g_taps.copy()
        dropped[-1] = 0
        differ(dropped, g_taps, "last tap dropped: g_taps", R.GRAD_BAR)
    for off in (-1, 1):
        # an off-by-one lead on the same taps: padded with one zero tap where the lead leaves [0, K)
        wt = np.concatenate([[0.0], taps, [0.0]])
        wy = R.lti_fir(ex, wt, lead + 1 + off)
        differ(wy, y, f"lead {off:+d}: y", R.FWD_BAR)
        wgx, wgt = R.lti_fir_grads(gy, ex, wt, lead + 1 + off)
        differ(wgx, g_ex, f"lead {off:+d}: g_ex", R.GRAD_BAR)
        differ(wgt[1:-1], g_taps, f"lead {off:+d}: g_taps", R.GRAD_BAR)


@pytest.mark.parametrize("case", [c for c in LTI_ALL if (c[1] % 960) % 4], ids=str)
def test_lti_inputs_see_an_omitted_ragged_tail(case):
    """g_taps without the < 4 samples that follow the last full group of 4 in a 960-sample stretch."""
    B, T, K, lead = case
    ex, taps, gy = R.lti_inputs(*case)
    cut = gy.copy()
    for t0 in range(0, T, 960):
        n = min(960, T - t0)
        cut[:, t0 + (n & ~3): t0 + n] = 0
    differ(R.lti_fir_grads(cut, ex, taps, lead)[1], lti_ref(case)[2], f"ragged tail omitted {case}", R.GRAD_BAR)


@pytest.mark.parametrize("cid,causal", FRAME_IDS)
def test_frames_inputs_see_wrong_kernels(cid, causal):
    c = R.frames_inputs(cid, causal)
    ex, kern, gy, hop, f0, N, F, nfr = (c[k] for k in ("ex", "kern", "gy", "hop", "frame0", "N", "F", "nfr"))
    y, g_ex, g_kern = frames_ref(cid, causal)
    grads = hop % 4 == 0
    mirrored = kern[:, :, ::-1]
    differ(R.frames_fir(ex, mirrored, hop, causal, f0), y, "row mirrored: y", R.FWD_BAR)
    short = kern.copy()
    short[:, :, -1] = 0
    # the last tap multiplies a sample at all (not where the excitation is shorter than the kernel: the largest-N case, N = 505
    # and the hops of 1 and 3 samples)
    last_seen = nfr * hop >= N if causal else N - 1 - (N - 1) // 2 < c["T"]
    assert last_seen or cid in ("pass-N505", "odd-hop1", "odd-hop3", "largest-N"), cid
    if last_seen:
        differ(R.frames_fir(ex, short, hop, causal, f0), y, "last tap dropped: y", R.FWD_BAR)
    if grads:
        differ(R.frames_fir_grads(gy, ex, mirrored, hop, causal, f0)[0], g_ex, "row mirrored: g_ex", R.GRAD_BAR)
        differ(g_kern[:, :, ::-1], g_kern, "row mirrored: g_kern", R.GRAD_BAR)
    if grads and last_seen:
        differ(R.frames_fir_grads(gy, ex, short, hop, causal, f0)[0], g_ex, "last tap dropped: g_ex", R.GRAD_BAR)
        dropped = g_kern.copy()
        dropped[:, :, -1] = 0
        differ(dropped, g_kern, "last tap dropped: g_kern", R.GRAD_BAR)
    if f0 > 0:
        rolled = np.roll(kern, f0, axis=1)                 # rolled[f + f0] = kern[f]: what reading row f would apply
        differ(R.frames_fir(ex, rolled, hop, causal, f0), y, "row f for f + frame0: y", R.FWD_BAR)
        differ(R.frames_fir_grads(gy, ex, rolled, hop, causal, f0)[0], g_ex, "row f for f + frame0: g_ex", R.GRAD_BAR)
        differ(np.roll(g_kern, -f0, axis=1), g_kern, "row f for f + frame0: g_kern", R.GRAD_BAR)
    if grads and f0 + nfr < F:
        stale = g_kern.copy()
        stale[:, f0 + nfr] = g_kern[:, f0 + nfr - 1]                            # an unused frame's gradient left non-zero
        differ(stale, g_kern, "unused row not zero: g_kern", R.GRAD_BAR)
    if grads and R.frames_reach(c) < c["T"]:
        assert np.all(g_ex[:, R.frames_reach(c):] == 0) and np.any(g_ex[:, R.frames_reach(c) - 1] != 0)


@pytest.mark.parametrize("case", R.DECIM_CASES + R.DECIM_ADJ_CASES, ids=str)
def test_decimator_inputs_see_wrong_kernels(case):
    os_, K, N = case
    x, taps, g = R.decim_inputs(*case)
    K = taps.shape[0]
    y, gx = decim_ref(case)
    for off in (-1, 1):                                  # polyphase offset half +- 1: the same taps one sample early / late
        wt = np.concatenate([[0.0, 0.0], taps, [0.0, 0.0]])
        wt = np.roll(wt, off)
        differ(R.decimate(x, wt, os_), y, f"half {off:+d}: out", R.FWD_BAR)
        differ(R.decimate_adjoint(g, wt, os_, N), gx, f"half {off:+d}: adjoint", R.GRAD_BAR)
    half = (K - 1) // 2
    if case[1] not in (None, 1) and N > half:            # random taps, and the last one reaches a sample of output 0 at all
        short = taps.copy()
        short[-1] = 0
        differ(R.decimate(x, short, os_), y, "last tap dropped: out", R.FWD_BAR)
        differ(R.decimate_adjoint(g, short, os_, N), gx, "last tap dropped: adjoint", R.GRAD_BAR)


def test_designed_taps_cannot_see_a_dropped_last_tap():
    """Why the dropped-tap check above runs on the random taps (os 5 and 8) only: the last tap of the designed low-pass is
    some 1e-5 of the largest one, below what the bar resolves.  The random-tap cases cover that mistake."""
    for os_ in (2, 3, 4):
        t = R.decimator_taps(os_)
        assert abs(t[-1]) < 1e-3 * np.abs(t).max()
    assert any(K not in (None, 1) for _, K, _ in R.DECIM_CASES)


# ------------------------------------------------------------------------------------------------ float32 emulation
@pytest.mark.parametrize("case", LTI_ALL, ids=str)
def test_lti_sequential_fp32(case):
    ex, taps, gy = R.lti_inputs(*case)
    y, g_ex, g_taps = lti_ref(case)
    within_third(R.lti_fir_f32(ex, taps, case[3]), y, f"lti {case} y", R.FWD_BAR)
    e_ex, e_taps = R.lti_fir_grads_f32(gy, ex, taps, case[3])
    within_third(e_ex, g_ex, f"lti {case} g_ex", R.GRAD_BAR)
    within_third(e_taps, g_taps, f"lti {case} g_taps", R.GRAD_BAR)


@pytest.mark.parametrize("cid,causal", FRAME_IDS)
def test_frames_sequential_fp32(cid, causal):
    c = R.frames_inputs(cid, causal)
    y, g_ex, g_kern = frames_ref(cid, causal)
    within_third(R.frames_fir_f32(c["ex"], c["kern"], c["hop"], causal, c["frame0"]), y, f"frames {cid} y", R.FWD_BAR)
    if c["hop"] % 4 == 0:
        e_ex, e_kern = R.frames_fir_grads_f32(c["gy"], c["ex"], c["kern"], c["hop"], causal, c["frame0"])
        within_third(e_ex, g_ex, f"frames {cid} g_ex", R.GRAD_BAR)
        within_third(e_kern, g_kern, f"frames {cid} g_kern", R.GRAD_BAR)


@pytest.mark.parametrize("case", R.DECIM_CASES + R.DECIM_ADJ_CASES, ids=str)
def test_decimator_sequential_fp32(case):
    os_, K, N = case
    x, taps, g = R.decim_inputs(*case)
    y, gx = decim_ref(case)
    within_third(R.decimate_f32(x, taps, os_), y, f"decimate {case}", R.FWD_BAR)
    within_third(R.decimate_adjoint_f32(g, taps, os_, N), gx, f"decimate adjoint {case}", R.GRAD_BAR)


# ------------------------------------------------------------------------------------------------ the cases themselves
def test_the_cases_cover_what_they_are_named_for():
    """From the kernels' own launch arithmetic (csrc/noise_fir.hip: tiles of 252 outputs, stretches of 960 samples)."""
    grid = {(-(-T // 960), -(-K // 252)) for _, T, K, _ in R.LTI_CASES}
    assert (2, 1) in grid and (3, 2) in grid and (4, 3) in grid
    assert {(T % 960) % 4 for _, T, _, _ in R.LTI_CASES} == {0, 1, 2, 3}
    assert any(T < K for _, T, K, _ in R.LTI_CASES) and any(T == 252 for _, T, _, _ in R.LTI_CASES)
    assert {lead for _, _, K, lead in R.LTI_CASES if K == 264} == {0, 101, 263}
    ns = {c["N"] for c in R.FRAMES_CASES.values()}
    assert {n % 4 for n in ns} == {0, 1, 2, 3} and {251, 252, 253, 505} <= ns
    assert {-(-c["hop"] // 252) for c in R.FRAMES_CASES.values() if c["N"] == 30 and c["hop"] > 200} == {1, 2, 3}
    for causal in (False, True):
        assert R.frames_inputs("one-frame", causal)["nfr"] == 1
        c = R.frames_inputs("unused-rows", causal)
        assert c["F"] == c["nfr"] + 3
        c = R.frames_inputs("long-tail", causal)
        assert c["nfr"] == c["F"] and c["T"] - R.frames_reach(c) > 600
        for f0 in (0, 1, 2):
            c = R.frames_inputs(f"frame0-{f0}", causal)
            assert c["nfr"] == 3 and f0 + c["nfr"] < c["F"]
        c = R.frames_inputs("many-frames", causal)
        assert (c["N"] - 1 + c["hop"] - 1) // c["hop"] + 1 >= 14        # frames whose support reaches one 4-sample tile
    for os_ in (2, 3, 4, 5):
        assert {(N - 1) // os_ + 1 for N in R.decim_lengths(os_)} >= {1, 2, 1024, 1025}
    # the os = 4 fill test: three tiles of 1024 outputs, the middle one interior (its whole staged span inside the signal)
    os_, _, N = R.DECIM_FILL
    K = R.decimator_taps(os_).shape[0]
    half = (K - 1) // 2
    dmin, dmax = -((half + os_ - 1) // os_), half // os_
    span = 1024 + ((dmax - dmin + 1 + 2) // 4) * 4 + 4
    interior = [o0 for o0 in range(0, (N - 1) // os_ + 1, 1024) if (o0 + dmin) * os_ >= 0 and (o0 + dmin + span) * os_ <= N]
    assert -(-((N - 1) // os_ + 1) // 1024) == 3 and interior == [1024]


def test_oversize_filters_are_refused_on_the_host():
    """The dynamic-LDS bound of the packed-FIR launches is checked before anything is launched: with host pointers and no
    device at all, the calls come back GOLF_EUNSUPPORTED naming LDS and the largest accepted size."""
    from golf_amd import _lib

    lib = _lib.load()
    buf = torch.zeros(8192)
    p = buf.data_ptr()
    calls = {
        "ntaps": lambda: lib.golf_lti_fir_f32(p, 400, p, 3840, 0, p, 400, 1, 300, None),
        "reversed ntaps": lambda: lib.golf_lti_fir_f32(p, 400, p, -3840, 0, p, 400, 1, 300, None),
        "N": lambda: lib.golf_ltv_fir_frames_fwd_f32(p, 400, p, 3840, p, 400, 1, 300, 1, 3837, 8, 0, None),
        "causal N": lambda: lib.golf_ltv_fir_frames_causal_fwd_f32(p, 400, p, 3840, p, 400, 1, 300, 1, 3840, 8, 0, None),
        "hop": lambda: lib.golf_ltv_fir_frames_bwd_f32(p, 4000, p, 4000, p, 8, p, 4000, p, 1, 4000, 1, 8, 3840, 0, None),
        "causal hop": lambda: lib.golf_ltv_fir_frames_causal_bwd_f32(p, 4000, p, 4000, p, 8, p, 4000, p, 1, 4000, 1, 8, 3840,
                                                                     0, None),
    }
    for what, call in calls.items():
        rc = call()
        msg = lib.golf_last_error().decode()
        print(f"{what}: rc {rc}: {msg}")
        assert rc < 0 and "LDS" in msg and "3836" in msg, (what, rc, msg)
        with pytest.raises(_lib.GolfError, match="LDS"):
            _lib.check(rc, what)
