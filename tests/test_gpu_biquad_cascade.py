"""The cascaded-biquad frame filter (csrc/lpc_ff.hip: ff_biquad_frames_kernel, ff_biquad_bwd_kernel,
ff_biquad_bwd_ola_kernel, through golf_amd.functional.biquad_frames_ola) on every lane count, frame count, window length
and staging size at which the kernels take another path, forward and all three gradients against the float64 oracle.

The bound is the project's convention for recursions: 1e-4 + 3 x what the same cascade loses in sequential float32 on the
same input (tests/biquad_ref.py::cascade_f32; tests/test_biquad_ref_host.py holds that to 1e-4 on every default case, so the
bound never exceeds 4e-4).  The gradients use the bound of their case's forward."""
import functools

import numpy as np
import pytest
import torch

import biquad_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.array(x, dtype=np.float32)).cuda()   # a copy: the shared cases are read-only arrays


@functools.lru_cache(maxsize=None)
def reference(cid):
    """(case, gy, (y, g_ex, g_gain, g_biquads) of the float64 oracle, bound): computed once per case, shared, read-only."""
    from oracle import golf_oracle as O

    c = R.case(cid)
    args = (c["ex"], c["gain"], c["bq"], c["hop"], c["win"])
    kw = dict(pad=c["pad"], frame_gain=c["frame_gain"])
    ref = O.biquad_frames_ola_forward(*args, **kw)
    gy = R.make_gy(ref, c["seed"])
    refs = (ref,) + tuple(O.biquad_frames_ola_backward(gy, *args, **kw))
    e32 = rel_err(R.cascade_f32(*args, **kw), ref)[0]
    for v in (gy,) + refs:
        v.setflags(write=False)
    return c, gy, refs, (1e-4 + 3 * e32, e32)


def run(ex, gain, bq, win, hop, pad, frame_gain, gy=None, poison=False):
    """y or, with gy, (y, g_ex, g_gain, g_biquads) as numpy arrays.  ``poison`` releases NaN-filled blocks of the sizes of
    the backward's four outputs to the caching allocator right before the backward."""
    from golf_amd import functional as GF

    t = [v if torch.is_tensor(v) else dev(v) for v in (ex, gain, bq)]
    if gy is None:
        y = GF.biquad_frames_ola(t[0], t[1], t[2], dev(win), hop, pad=pad, frame_gain=frame_gain)
        torch.cuda.synchronize()
        return y.cpu().numpy()
    t = [v.requires_grad_(True) for v in t]
    y = GF.biquad_frames_ola(t[0], t[1], t[2], dev(win), hop, pad=pad, frame_gain=frame_gain)
    gyd = dev(gy)
    if poison:
        blocks = [torch.full(v.shape, float("nan"), device="cuda") for v in t for _ in range(3)]
        torch.cuda.synchronize()
        del blocks
    (y * gyd).sum().backward()
    torch.cuda.synchronize()
    return (y.detach().cpu().numpy(),) + tuple(v.grad.cpu().numpy() for v in t)


def run_case(c, gy=None, **kw):
    return run(c["ex"], c["gain"], c["bq"], c["win"], c["hop"], c["pad"], c["frame_gain"], gy, **kw)


def check(got, want, what, bound):
    emax, el2 = rel_err(got, want)
    print(f"{what}: rel-max {emax:.3e} rel-l2 {el2:.3e} (bound {bound:.3e})")
    assert np.isfinite(got).all(), what
    assert emax <= bound and el2 <= bound, (what, emax, el2, bound)


NAMES = ("y", "g_ex", "g_gain", "g_biquads")


def check_case(cid):
    c, gy, refs, (bound, e32) = reference(cid)
    outs = run_case(c, gy, poison=True)
    print(f"{cid}: sequential fp32 cascade rel-max {e32:.3e}")
    for name, got, want in zip(NAMES, outs, refs):
        assert got.shape == want.shape, (cid, name, got.shape, want.shape)
        check(got, want, f"{cid} {name}", bound)
    # what no frame reaches: exact zeros, whatever the allocator handed out
    y, g_ex, g_gain, g_bq = outs
    assert np.all(g_bq[:, c["nfr"]:] == 0), "g_biquads of the frames beyond nfr"
    assert np.all(g_ex[:, c["used"]:] == 0), "g_ex past the last used sample"
    if c["frame_gain"]:
        assert np.all(g_gain[:, c["nfr"]:] == 0), "g_gain of the frames beyond nfr"
    return outs, e32


@pytest.mark.parametrize("cid", list(R.FRAME_GAIN_SHAPES))
def test_frame_gain_shapes(cid):
    check_case(cid)


@pytest.mark.parametrize("cid", list(R.INTERP_GAIN_SHAPES))
def test_interpolated_gain_shapes(cid):
    check_case(cid)


@pytest.mark.parametrize("cid", list(R.HARSH_SHAPES))
def test_conditioning(cid):
    """Poles up to radius 0.99 and logits of sigma 1.0: the same bound formula; the fp32 yardstick may not exceed 1e-3
    (a bound looser than 3.1e-3 would prove nothing: another seed then).

    The backward carries its recursion state in float64 for this case's sake: with an fp32 state the gain gradient of one
    frame of harsh-K16-W200 came out 2.7 % off (g_gain rel-max 1.6e-3 against the bound of 1.42e-3), and a CPU restatement
    of the same backward ranged from 2.7e-4 to 2.3e-3 with nothing but the order of the fp32 operations changed."""
    _, e32 = check_case(cid)
    assert e32 <= 1e-3, (cid, e32)


@pytest.mark.parametrize("cid", ["K2-nfr2-extraF-ragged-blocks9", "K6-W2hop-unused-tail", "K4-full-wave-W96-blocks25",
                                 "K3-F6-nfr4-W16-extraF"])
def test_frames_beyond_nfr_and_the_unused_tail_are_zero(cid):
    """F > nfr and an excitation longer than the frames reach, three times over with NaN-filled blocks of the gradients'
    sizes released right before every backward: the zeros are written, not inherited."""
    c, gy, refs, _ = reference(cid)
    assert c["F"] > c["nfr"]
    for _ in range(3):
        y, g_ex, g_gain, g_bq = run_case(c, gy, poison=True)
        assert np.isfinite(g_ex).all() and np.isfinite(g_gain).all() and np.isfinite(g_bq).all()
        assert np.all(g_bq[:, c["nfr"]:] == 0) and np.abs(g_bq[:, : c["nfr"]]).min() > 0
        assert np.all(g_ex[:, c["used"]:] == 0) and np.abs(g_ex[:, : c["used"]]).sum() > 0
        if c["frame_gain"]:
            assert np.all(g_gain[:, c["nfr"]:] == 0) and np.abs(g_gain[:, : c["nfr"]]).min() > 0
    assert cid != "K6-W2hop-unused-tail" or c["Tx"] - c["used"] == 5


@pytest.mark.parametrize("cid", ["K3-nfr3-W50-blocks13", "K11-nfr7-W160-blocks43", "K7-F15-W100",
                                 "K3-F4-W16-excitation-past-the-gain"])
def test_row_strided_excitation_is_bit_identical(cid):
    """The excitation as a column slice of a wider tensor (row stride > width) whose other columns hold NaN: forward and
    gradients bit-identical to the contiguous call, and nothing outside the slice is read or given a gradient."""
    c, gy, _, _ = reference(cid)
    want = run_case(c, gy)
    Tx = c["Tx"]
    wide = torch.full((c["B"], Tx + 11), float("nan"), device="cuda")
    wide[:, 3: 3 + Tx] = dev(c["ex"])
    wide.requires_grad_(True)
    view = wide[:, 3: 3 + Tx]
    assert view.stride(0) == Tx + 11 and not view.is_contiguous()
    from golf_amd import functional as GF

    gain, bq = dev(c["gain"]).requires_grad_(True), dev(c["bq"]).requires_grad_(True)
    y = GF.biquad_frames_ola(view, gain, bq, dev(c["win"]), c["hop"], pad=c["pad"], frame_gain=c["frame_gain"])
    (y * dev(gy)).sum().backward()
    torch.cuda.synchronize()
    g_wide = wide.grad.cpu().numpy()
    got = (y.detach().cpu().numpy(), g_wide[:, 3: 3 + Tx], gain.grad.cpu().numpy(), bq.grad.cpu().numpy())
    for name, a, b in zip(NAMES, got, want):
        assert np.array_equal(a, b), (cid, name, np.abs(a - b).max())
    assert np.all(g_wide[:, :3] == 0) and np.all(g_wide[:, 3 + Tx:] == 0)


@pytest.mark.parametrize("K", [1, 2, 3])
def test_direct_form_kernel_agrees(K):
    """Interpolated gain, orders 2, 4, 6: the sections multiplied out in float64 and run through the direct-form kernel
    (GF.lti_frames_ola, another kernel family).  Both GPU results and the oracle agree within 1e-4; a direct form of
    order <= 6 with poles inside 0.95 loses nothing that matters in fp32."""
    from golf_amd import functional as GF
    from golf_amd.utils import biquads2lpc
    from oracle import golf_oracle as O

    B, hop, W, F = 2, 16, 64, 6
    ex, gain, bq, win, pad = R.make_case(B, K, hop, W, F, 0, 0, False, seed=50 + K)
    # the direct form is monic and this gain is interpolated between frames, so 1 / prod(a0) folds into the gain only
    # if it is the same in every frame: section k gets a0 = a0k[k] everywhere
    a0k = np.linspace(0.8, 1.25, K + 2)[1:-1].astype(np.float32)
    bq = (bq / bq[..., :1] * a0k[:, None]).astype(np.float32)
    ref = O.biquad_frames_ola_forward(ex, gain, bq, hop, win, pad=pad, frame_gain=False)
    y = run(ex, gain, bq, win, hop, pad, False)
    bq64 = torch.from_numpy(bq).double()
    lpc = biquads2lpc(bq64 / bq64[..., :1])
    yd = GF.lti_frames_ola(dev(ex), dev(gain.astype(np.float64) / np.prod(a0k.astype(np.float64))), dev(lpc.numpy()),
                           dev(win), hop)
    yd = yd.cpu().numpy()
    assert y.shape == yd.shape == ref.shape
    check(y, ref, f"K{K} cascade vs oracle", 1e-4)
    check(yd, ref, f"K{K} direct form vs oracle", 1e-4)
    check(y, yd, f"K{K} cascade vs direct form", 1e-4)


@pytest.mark.parametrize("K", [1, 16])
def test_identity_sections_give_x_times_gain(K):
    """Sections (1, 0, 0) filter nothing, and the overlap-add of the windowed frames over the overlap-add of the window is
    a partition of unity: y = ex * upsampled gain.  One product, K exact pass-throughs, at most 4 window products summed
    and one division: a few ulp, 1e-6 relative."""
    from oracle import golf_oracle as O

    B, hop, W, F = 2, 16, 64, 7
    ex, gain, bq, win, pad = R.make_case(B, K, hop, W, F, 0, 0, False, seed=60 + K)
    bq = np.zeros_like(bq)
    bq[..., 0] = 1
    y = run(ex, gain, bq, win, hop, pad, False)
    G = O.linear_upsample(gain, hop)
    check(y, ex[:, : y.shape[1]] * G[:, : y.shape[1]], f"K{K} identity sections", 1e-6)


def test_scaling_a_section_scales_the_output():
    """(a0, a1, a2) -> c (a0, a1, a2) on one section divides the output by c.  c = 4 keeps a1/a0 and a2/a0 bit-identical in
    any fp32 formulation, so the recursion is the same and only the output scale moves: 1e-6 relative, K = 1 and the middle
    and last sections of K = 16."""
    c4 = 4.0
    for cid, ks in (("K1-one-frame-W8-blocks2", (0,)), ("K16-whole-row-W200-blocks54", (0, 7, 15))):
        c, _, _, _ = reference(cid)
        y = run_case(c)
        for k in ks:
            bq = c["bq"].copy()
            bq[:, :, k, :] *= c4
            ys = run(c["ex"], c["gain"], bq, c["win"], c["hop"], c["pad"], c["frame_gain"])
            check(ys * c4, y, f"{cid} section {k} times {c4}", 1e-6)
            assert np.abs(ys).max() < 0.3 * np.abs(y).max()


@pytest.mark.parametrize("cid", ["K2-nfr2-extraF-ragged-blocks9", "K11-nfr7-W160-blocks43", "K16-whole-row-W200-blocks54",
                                 "K16-F5-W48"])
def test_sections_commute(cid):
    """LTI sections commute: reversing and rotating the sections of every frame moves the output by no more than two fp32
    cascades may differ, the bound of the shape tests."""
    c, _, refs, (bound, _) = reference(cid)
    y = run_case(c)
    K = c["K"]
    for perm in (np.arange(K)[::-1], np.roll(np.arange(K), 1), np.random.default_rng(K).permutation(K)):
        yp = run(c["ex"], c["gain"], np.ascontiguousarray(c["bq"][:, :, perm]), c["win"], c["hop"], c["pad"], c["frame_gain"])
        check(yp, y, f"{cid} sections {perm.tolist()} vs in order", bound)
        check(yp, refs[0], f"{cid} sections {perm.tolist()} vs oracle", bound)


@pytest.mark.parametrize("cid,Ks", [("K3-nfr3-W50-blocks13", (4, 9, 16)), ("K11-nfr7-W160-blocks43", (12, 16)),
                                    ("K5-F4-W32-blocks9", (6, 16))])
def test_appended_identity_sections_change_nothing(cid, Ks):
    """K -> K + j sections, the new ones (1, 0, 0): a lane with a1 = a2 = 0 and gain 1 passes its input on exactly, in the
    forward and in the adjoint, so output and the real sections' gradients stay within 1e-6 relative (the pipeline is j
    steps longer, the block count and its parity change, the write-out moves to another lane)."""
    c, gy, _, _ = reference(cid)
    want = run_case(c, gy)
    K = c["K"]
    for K2 in Ks:
        bq = np.zeros(c["bq"].shape[:2] + (K2, 3), dtype=np.float32)
        bq[..., 0] = 1
        bq[:, :, :K] = c["bq"]
        got = run(c["ex"], c["gain"], bq, c["win"], c["hop"], c["pad"], c["frame_gain"], gy)
        for name, a, b in zip(NAMES, got, want):
            check(a[:, :, :K] if name == "g_biquads" else a, b, f"{cid} K {K} -> {K2} {name}", 1e-6)


@pytest.mark.parametrize("cid", ["K8-nfr5-W30-blocks10", "K16-F5-W48", "K12-F8-W480-XS880", "K7-F15-W100"])
def test_same_call_twice_is_bit_identical(cid):
    c, gy, _, _ = reference(cid)
    first, second = run_case(c, gy), run_case(c, gy, poison=True)
    for name, a, b in zip(NAMES, first, second):
        assert np.array_equal(a, b), (cid, name)


def test_small_call_after_a_large_one():
    """K = 2, W = 32 first, then K = 16, W = 904 (which fills the LDS up to its limits and a large workspace), then the small
    call again: bit-identical.  Nothing of the large call's LDS, workspace or staged tail reaches the small one."""
    small, gs, _, _ = reference("K2-nfr2-extraF-ragged-blocks9")
    large, gl, _, _ = reference("K16-W904-XS1664-bwd-lds-65376")
    first = run_case(small, gs)
    run_case(large, gl)
    after = run_case(small, gs)
    for name, a, b in zip(NAMES, first, after):
        assert np.array_equal(a, b), name


# ---- the documented refusals: host-side argument checks that raise GolfError before any launch ------------------------------
def _good_call():
    c, gy, refs, (bound, _) = reference("K2-nfr2-extraF-ragged-blocks9")
    outs = run_case(c, gy)
    for name, got, want in zip(NAMES, outs, refs):
        check(got, want, f"after the refusal: {name}", bound)


def _refused(match, B=1, K=2, hop=8, W=32, F=3, Tx=None, frame_gain=True, pad=None, backward=False):
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError

    pad = ((W - hop) // 2 if frame_gain else W // 2) if pad is None else pad
    Tx = ((F - 1) * hop + W - 2 * pad if frame_gain else (F - 1) * hop + 1) if Tx is None else Tx
    bq = torch.zeros(B, F, K, 3, device="cuda")
    bq[..., 0] = 1
    ex, gain = torch.randn(B, Tx, device="cuda"), torch.ones(B, F, device="cuda")
    win = torch.hann_window(W, device="cuda")
    if not backward:
        with pytest.raises(GolfError, match=match):
            GF.biquad_frames_ola(ex, gain, bq, win, hop, pad=pad, frame_gain=frame_gain)
    else:
        bq.requires_grad_(True)
        y = GF.biquad_frames_ola(ex, gain, bq, win, hop, pad=pad, frame_gain=frame_gain)   # the forward has room
        assert torch.isfinite(y).all()
        with pytest.raises(GolfError, match=match):
            y.sum().backward()
        assert bq.grad is None
    torch.cuda.synchronize()
    _good_call()


def test_refuses_17_sections():
    _refused(r"17 sections > 16 \(one DPP row per frame\)", K=17)


def test_refuses_a_hop_that_is_no_multiple_of_4():
    _refused("hop=6 must be a multiple of 4", hop=6, W=24)


def test_refuses_an_interpolated_gain_of_one_frame():
    _refused("interpolated gain needs F >= 2", F=1, frame_gain=False)


def test_refuses_more_frames_than_coefficient_frames():
    _refused("4 frames for 3 coefficient frames", F=3, Tx=3 * 8 + 8)


def test_refuses_a_forward_beyond_its_lds_staging():
    # 4 * (3*hop + 5*W + 168) = 70592 bytes > 60 KB
    _refused("window 3040 too long for the LDS staging", hop=760, W=3040, F=2)


def test_backward_lds_limit():
    """(K + 2) * (W + 4) * 4 <= 65536: K = 15, W = 960 (65552 bytes) computes a forward and refuses to train, saying so;
    K = 14, W = 960 (61696 bytes) trains (tests/biquad_ref.py harsh-K14-W960, checked against the oracle in
    test_conditioning, and once more here on the identity sections: every gradient finite, g_ex = gain * gy)."""
    from golf_amd import functional as GF

    _refused("15 sections x window 960 exceed the LDS staging", K=15, hop=240, W=960, F=2, backward=True)
    B, F, K, hop, W = 1, 2, 14, 240, 960
    bq = torch.zeros(B, F, K, 3, device="cuda")
    bq[..., 0] = 1
    bq.requires_grad_(True)
    ex = torch.randn(B, hop + W - 2 * ((W - hop) // 2), device="cuda", requires_grad=True)
    gain = torch.full((B, F), 0.5, device="cuda")
    y = GF.biquad_frames_ola(ex, gain, bq, torch.hann_window(W, device="cuda"), hop)
    y.sum().backward()
    torch.cuda.synchronize()
    assert torch.isfinite(bq.grad).all() and bq.grad.abs().sum() > 0
    # constant gain: y = 0.5 * ex exactly up to the partition of unity, so d sum(y) / d ex = 0.5
    assert torch.allclose(ex.grad, torch.full_like(ex.grad, 0.5), rtol=1e-5, atol=0)
