"""The sample-wise LTV all-pole filter with its recursion in float64 (csrc/lpc_any.hip): double tensors, and fp32 tensors
with ``mode="fp64"``, against the float64 oracle -- forward, carried state, all gradients, gradcheck.

Bars.  Double tensors: 1e-10 relative (max-norm and L2).  A sequential fp32 emulation sits at <= 6e-6 on exactly these
inputs (tests/test_gpu_lpc_ss_anyshape.py), an amplification of ~100 over 2^-24, so the same recursion in double belongs
near 1e-14; 1e-10 leaves four orders for summation-order differences against numpy and is still three orders below what
ONE fp32 temporary on the chain (>= 6e-8) would produce.  ``mode="fp64"`` on fp32 tensors: y within 1e-6 (the store rounds
once, 2^-24 ~ 6e-8 of the sample), gradients within 1e-5 (they read the STORED fp32 y, so its rounding enters the
correlation sums).  Ill-conditioned rows (sequential fp32 beyond 1e-4): mode="fp64" <= 1e-6 on every row, double <= 1e-8
(an e_seq up to 5e-3 scaled by 2^-29 is 1e-11).  Blocks chained through the state: the BITS of the one-shot call; their
gradients within 1e-10 of the one-shot's in double and, on fp32 tensors, within the 1e-5 of that mode's gradients (the
cotangent of the state is added into an fp32 gy).

Measured on MI355X (worst over the cases of this file; each test prints its own figures):
  double tensors      y 9.5e-15   g_ex 7.0e-15   g_gain 7.0e-15   g_a 5.9e-15   (with a state: y 4.3e-15, zf 6.2e-15,
                      g_a 8.0e-15, g_zi 4.1e-15)
  mode="fp64" / fp32  y 4.5e-8    g_ex 4.7e-8    g_gain 4.0e-8    g_a 6.1e-8    (with a state: y 5.6e-8, g_a 6.3e-8,
                      g_zi 6.4e-8) -- every gradient under 1e-6
  ill-conditioned     rows 10, 31, 0, 1: sequential fp32 2.6e-4, 6.4e-5, 1.5e-6, 1.1e-6;  mode="fp64" 5.1e-8, 3.6e-8,
                      3.3e-8, 4.2e-8;  double tensors 6.9e-13, 1.3e-13, 3.8e-15, 2.4e-15
  blocks vs one-shot  gradients: double 5.6e-15, mode="fp64" 1.3e-7
"""
import numpy as np
import pytest
import torch

from conftest import rel_err
from test_gpu_lpc_ss_anyshape import case, smooth_case
from test_lpc_ss_state_host import torch_ref_grads

pytestmark = pytest.mark.gpu

TOL64 = 1e-10
TOL_MODE_Y = 1e-6
TOL_MODE_G = 1e-5

SHAPES = [
    (2, 9, 22, 100, None, 0.5),
    (2, 9, 22, 240, None, 0.5),      # on the ring grid: the double path serves it too
    (2, 5, 40, 441, None, 0.25),
    (2, 6, 64, 96, None, 0.25),      # all 64 lanes are taps
    (2, 4, 64, 7, None, 0.25),       # hop << M, T = 22 < M
    (1, 4, 5, 3, None, 0.5),
    (2, 5, 1, 16, None, 0.5),        # M = 1
    (2, 200, 5, 1, None, 0.5),       # hop 1
    (1, 1, 4, 7, None, 0.5),         # F = 1
    (3, 10, 22, 100, 777, 0.5),      # ends inside a frame
    (3, 10, 22, 100, 1200, 0.5),     # the excitation's tail: its gradient is exactly 0
    (9, 4, 12, 50, None, 0.5),
] + [(1, 20, 22, 16, Tx, 0.5) for Tx in (63, 64, 65, 129)]   # I/O-block edges


def dev(x, dtype):
    """The fp32-drawn numbers on the device, widened (exactly) for torch.float64."""
    return torch.as_tensor(np.array(x)).cuda().to(dtype)


def check(x, ref, what, tol):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
    emax, el2 = rel_err(x, ref)
    print(f"{what}: rel-max {emax:.3e} rel-l2 {el2:.3e}")
    assert np.isfinite(x).all(), what
    assert emax <= tol and el2 <= tol, (what, emax, el2)


def leaves(arrays, dtype, grads=None):
    grads = (True,) * len(arrays) if grads is None else grads
    return [dev(v, dtype).requires_grad_(g) for v, g in zip(arrays, grads)]


def run(ex, gain, a, gy, hop, dtype, grads=(True, True, True), **kw):
    from golf_amd import functional as GF

    t = leaves((ex, gain, a), dtype, grads)
    y = GF.ltv_allpole_ss(t[0], t[1], t[2], hop, **kw)
    (y * dev(gy, dtype)).sum().backward()
    torch.cuda.synchronize()
    return (y.detach(),) + tuple(v.grad for v in t)


@pytest.mark.parametrize("B,F,M,hop,Tx,scale", SHAPES)
def test_double_tensors_vs_oracle(B, F, M, hop, Tx, scale):
    ex, gain, a, gy, T, refs = case(B, F, M, hop, Tx, scale)
    out = run(ex, gain, a, gy, hop, torch.float64, mode="chunked")   # (a mode of the fp32 scan is ignored, as off the grid)
    assert out[0].shape == (B, T) and out[1].shape == ex.shape
    for v, r, what in zip(out, refs, ("y", "g_ex", "g_gain", "g_a")):
        assert v.dtype == torch.float64
        check(v, r, what, TOL64)
    if ex.shape[1] > T:
        assert torch.equal(out[1][:, T:], torch.zeros_like(out[1][:, T:]))
    again = run(ex, gain, a, gy, hop, torch.float64, mode="fp64")    # the same as no mode
    for u, v in zip(out, again):
        assert torch.equal(u, v)


@pytest.mark.parametrize("B,F,M,hop,Tx,scale", SHAPES)
def test_fp64_mode_on_fp32_tensors_vs_oracle(B, F, M, hop, Tx, scale):
    ex, gain, a, gy, T, refs = case(B, F, M, hop, Tx, scale)
    out = run(ex, gain, a, gy, hop, torch.float32, mode="fp64")
    assert out[0].shape == (B, T) and out[1].shape == ex.shape
    for v, r, what, tol in zip(out, refs, ("y", "g_ex", "g_gain", "g_a"), (TOL_MODE_Y,) + (TOL_MODE_G,) * 3):
        assert v.dtype == torch.float32
        check(v, r, what + " (mode=fp64)", tol)
    if ex.shape[1] > T:
        assert torch.equal(out[1][:, T:], torch.zeros_like(out[1][:, T:]))


@pytest.mark.parametrize("io", [0, 1])
def test_tail_of_g_ex_is_written_into_a_poisoned_buffer(io):
    """The C entry itself, on a g_ex buffer full of NaN: every sample is overwritten and the tail is exactly 0."""
    from golf_amd import _lib
    from golf_amd import functional as GF

    B, F, M, hop, Tx = 3, 10, 22, 100, 1200
    ex, gain, a, gy, T, refs = case(B, F, M, hop, Tx, 0.5)
    dtype = torch.float64 if io else torch.float32
    ex_t, gain_t, a_t, gy_t = (dev(v, dtype) for v in (ex, gain, a, gy))
    y = GF.ltv_allpole_ss(ex_t, gain_t, a_t, hop, mode="fp64")
    width, stride = Tx, Tx + 9
    g_ex = torch.full((B, stride), float("nan"), dtype=dtype, device="cuda")
    g_gain = torch.full_like(gain_t, float("nan"))
    g_a = torch.full_like(a_t, float("nan"))
    lib = _lib.load()
    ws = GF._workspace(lib.golf_ltv_allpole_f64_workspace_bytes(B, T), "cuda")
    rc = lib.golf_ltv_allpole_bwd_f64(gy_t.data_ptr(), T, y.data_ptr(), T, ex_t.data_ptr(), Tx, gain_t.data_ptr(),
                                      a_t.data_ptr(), None, g_ex.data_ptr(), stride, width, g_gain.data_ptr(), g_a.data_ptr(),
                                      None, B, T, F, M, hop, ws.data_ptr(), ws.numel(), io, _lib.stream_ptr())
    _lib.check(rc, "golf_ltv_allpole_bwd_f64")
    torch.cuda.synchronize()
    assert torch.equal(g_ex[:, T:width], torch.zeros(B, width - T, dtype=dtype, device="cuda"))
    assert torch.isnan(g_ex[:, width:]).all()                       # and nothing beyond the width
    tol = TOL64 if io else TOL_MODE_G
    check(g_ex[:, :width], refs[1], "g_ex", tol)
    check(g_gain, refs[2], "g_gain", tol)
    check(g_a, refs[3], "g_a", tol)


_hard = {}


def hard_case():
    """Rows 10 and 31 (at the edge of stability) and two more of tests/test_gpu_lpc_ss.py::test_ill_conditioned_rows, at full
    length, with the oracle's forward."""
    if not _hard:
        from oracle import golf_oracle as O
        from test_gpu_lpc_ss import smooth_case as ss_smooth_case

        ex, gain, a = ss_smooth_case(48, 200, 22, 240, seed=40)
        rows = [10, 31, 0, 1]
        ex, gain, a = ex[rows], gain[rows], a[rows]
        ref = O.ltv_allpole_ss_forward(ex, gain, a, 240)
        for v in (ex, gain, a, ref):
            v.setflags(write=False)
        _hard["v"] = (ex, gain, a, ref)
    return _hard["v"]


def test_ill_conditioned_rows():
    """The point of the mode: rows on which the sequential fp32 recursion is beyond 1e-4 come out right."""
    from golf_amd import functional as GF
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import LTVMinimumPhaseFilterPrecise

    hop = 240
    ex, gain, a, ref = hard_case()
    scale = np.abs(ref).max(1)

    def row_err(y):
        return np.abs(y.detach().cpu().numpy() - ref).max(1) / scale

    f32 = [dev(v, torch.float32) for v in (ex, gain, a)]
    f64 = [dev(v, torch.float64) for v in (ex, gain, a)]
    e_seq = row_err(GF.ltv_allpole_ss(*f32, hop, mode="serial"))
    y_mode = GF.ltv_allpole_ss(*f32, hop, mode="fp64")
    e_mode = row_err(y_mode)
    e_dbl = row_err(GF.ltv_allpole_ss(*f64, hop))
    print("sequential fp32", e_seq, "mode=fp64", e_mode, "double", e_dbl)
    assert (e_seq > 1e-4).any(), "the case is supposed to contain ill-conditioned rows"
    assert y_mode.dtype == torch.float32
    assert np.all(e_mode <= 1e-6), e_mode
    assert np.all(e_dbl <= 1e-8), e_dbl
    filt = LTVMinimumPhaseFilterPrecise(lpc_order=22).cuda()
    filt.precision = "fp64"
    filt.health_check = True
    filt.prefetch(AudioTensor(f32[1], hop), AudioTensor(f32[2], hop))   # a no-op on this path
    assert getattr(filt, "_prepared", None) is None
    y_mod = filt(AudioTensor(f32[0]), AudioTensor(f32[1], hop), AudioTensor(f32[2], hop)).as_tensor()
    assert torch.equal(y_mod, y_mode)
    assert not filt.__dict__.get("_health_queue")                       # no status words on the float64 recursion
    y_mod64 = filt(AudioTensor(f64[0]), AudioTensor(f64[1], hop), AudioTensor(f64[2], hop)).as_tensor()
    assert y_mod64.dtype == torch.float64 and np.all(row_err(y_mod64) <= 1e-8)


def state_case(B, F, M, hop, scale):
    ex, gain, a, gy, T, _ = case(B, F, M, hop, None, scale)
    rng = np.random.default_rng(B + M)
    zi = rng.normal(0, 0.3, (B, M)).astype(np.float32)
    gzf = rng.normal(0, 1, (B, M)).astype(np.float32)
    return ex, gain, a, gy, T, zi, gzf


@pytest.mark.parametrize("B,F,M,hop,scale", [(2, 9, 22, 100, 0.5), (2, 4, 64, 7, 0.25)])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_initial_and_final_state_vs_oracle(B, F, M, hop, scale, dtype):
    from golf_amd import functional as GF
    from oracle import golf_oracle as O

    ex, gain, a, gy, T, zi, gzf = state_case(B, F, M, hop, scale)
    tol_y, tol_g = (TOL64, TOL64) if dtype == torch.float64 else (TOL_MODE_Y, TOL_MODE_G)
    G = O.linear_upsample(gain, hop)[:, :T]
    A = O.linear_upsample(a, hop)[:, :T]
    ref_y = O.sample_wise_lpc(ex[:, :T].astype(np.float64) * G, A, zi.astype(np.float64))
    t = leaves((ex, gain, a, zi), dtype)
    y, zf = GF.ltv_allpole_ss(t[0], t[1], t[2], hop, zi=t[3], return_zf=True, mode="fp64")
    assert y.dtype == dtype and zf.dtype == dtype and zf.shape == (B, M)
    check(y, ref_y, "y from zi", tol_y)
    ref = torch_ref_grads(ex, gain, a, hop, zi, gy, gzf)
    check(y, ref[0], "y from zi (torch restatement)", tol_y)
    check(zf, ref[1], "zf", tol_y)
    if T < M:   # the state shifts in behind the outputs
        assert torch.equal(zf[:, T:], t[3][:, :M - T])
    ((y * dev(gy, dtype)).sum() + (zf * dev(gzf, dtype)).sum()).backward()
    torch.cuda.synchronize()
    for v, r, what in zip(t, ref[2:], ("g_ex", "g_gain", "g_a", "g_zi")):
        assert v.grad.dtype == dtype
        check(v.grad, r, what + " with state", tol_g)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_blocks_are_the_bits_of_the_one_shot_call(dtype):
    from golf_amd import functional as GF

    B, F, M, hop = 2, 9, 22, 100
    ex, gain, a, gy, T, zi, gzf = state_case(B, F, M, hop, 0.5)
    gy_t, gzf_t = dev(gy, dtype), dev(gzf, dtype)

    def grads(fn):
        t = leaves((ex, gain, a, zi), dtype)
        y, zf = fn(*t)
        ((y * gy_t).sum() + (zf * gzf_t).sum()).backward()
        torch.cuda.synchronize()
        return [y.detach(), zf.detach()] + [v.grad for v in t]

    whole = grads(lambda x, g, c, z: GF.ltv_allpole_ss(x, g, c, hop, zi=z, return_zf=True, mode="fp64"))
    for n in (1, 2, 3):
        got = grads(lambda x, g, c, z: GF.ltv_allpole_ss_blocks(x, g, c, hop, n, zi=z, mode="fp64"))
        assert got[0].dtype == dtype and got[1].dtype == dtype
        assert torch.equal(got[0], whole[0]), n
        assert torch.equal(got[1], whole[1]), n
        for u, v, what in zip(got[2:], whole[2:], ("g_ex", "g_gain", "g_a", "g_zi")):
            check(u, v.cpu().numpy(), f"{what}, blocks of {n}", TOL64 if dtype == torch.float64 else TOL_MODE_G)
    # from zeros, truncated back-propagation: the same y
    with torch.no_grad():
        t = [dev(v, dtype) for v in (ex, gain, a)]
        y0 = GF.ltv_allpole_ss(*t, hop, mode="fp64")
        yb, zfb = GF.ltv_allpole_ss_blocks(*t, hop, 2, detach_state=True, mode="fp64")
        assert torch.equal(yb, y0) and torch.equal(zfb, y0[:, -M:].flip(1))


@pytest.mark.parametrize("F", [4, 1])
def test_gradcheck(F):
    from golf_amd import functional as GF

    B, M, hop = 2, 4, 5
    ex, gain, a = smooth_case(B, F, M, hop, seed=7)
    zi = np.random.default_rng(8).normal(0, 0.3, (B, M)).astype(np.float32)
    t = leaves((ex, gain, a, zi), torch.float64)
    assert torch.autograd.gradcheck(lambda x, g, c, z: GF.ltv_allpole_ss(x, g, c, hop, zi=z), t)
    assert torch.autograd.gradcheck(lambda x, g, c, z: GF.ltv_allpole_ss_blocks(x, g, c, hop, 1, zi=z), t)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_partial_grads(dtype):
    ex, gain, a, gy, T, _ = case(2, 9, 22, 100, None, 0.5)
    full = run(ex, gain, a, gy, 100, dtype, mode="fp64")[1:]
    for only in range(3):
        got = run(ex, gain, a, gy, 100, dtype, tuple(i == only for i in range(3)), mode="fp64")[1:]
        for i in range(3):
            if i == only:
                assert torch.equal(got[i], full[i])
            else:
                assert got[i] is None


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_strided_rows(dtype):
    from golf_amd import functional as GF

    B, F, M, hop = 2, 9, 22, 100
    ex, gain, a, gy, T, refs = case(B, F, M, hop, None, 0.5)
    tol_y, tol_g = (TOL64, TOL64) if dtype == torch.float64 else (TOL_MODE_Y, TOL_MODE_G)
    wide = torch.zeros(B, T + 37, device="cuda", dtype=dtype)
    wide[:, 5:5 + T] = dev(ex, dtype)
    wide.requires_grad_(True)
    _, gain_t, a_t = leaves((ex, gain, a), dtype)
    gy_wide = torch.zeros(B, T + 11, device="cuda", dtype=dtype)
    gy_wide[:, 3:3 + T] = dev(gy, dtype)
    gy_t = gy_wide[:, 3:3 + T]
    assert gy_t.stride(0) > T and wide[:, 5:5 + T].stride(0) > T
    y = GF.ltv_allpole_ss(wide[:, 5:5 + T], gain_t, a_t, hop, mode="fp64")
    y.backward(gy_t)
    torch.cuda.synchronize()
    check(y, refs[0], "y", tol_y)
    check(wide.grad[:, 5:5 + T], refs[1], "g_ex", tol_g)
    assert not wide.grad[:, :5].any() and not wide.grad[:, 5 + T:].any()
    check(gain_t.grad, refs[2], "g_gain", tol_g)
    check(a_t.grad, refs[3], "g_a", tol_g)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_two_runs_are_bit_equal(dtype):
    ex, gain, a, gy, T, _ = case(3, 10, 22, 100, 777, 0.5)
    first = run(ex, gain, a, gy, 100, dtype, mode="fp64")
    second = run(ex, gain, a, gy, 100, dtype, mode="fp64")
    for u, v in zip(first, second):
        assert torch.equal(u, v)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_forward_and_backward_capture_in_a_graph(dtype):
    from golf_amd import functional as GF

    hop = 100
    ex, gain, a, gy, T, _ = case(2, 9, 22, 100, None, 0.5)
    t = leaves((ex, gain, a), dtype)
    gy_t = dev(gy, dtype)

    def step():
        y = GF.ltv_allpole_ss(t[0], t[1], t[2], hop, mode="fp64")
        return (y,) + torch.autograd.grad(y, t, gy_t)

    eager = [v.detach().clone() for v in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                              # warm-up off the default stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for _ in range(2):
        for v in out:
            v.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(out, eager):
            assert torch.equal(u.detach(), v)


def test_status_raises_and_autocast_changes_nothing():
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError

    hop = 100
    ex, gain, a, gy, T, _ = case(2, 9, 22, 100, None, 0.5)
    f32 = [dev(v, torch.float32) for v in (ex, gain, a)]
    f64 = [v.double() for v in f32]
    st = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(GolfError, match="chunked"):
        GF.ltv_allpole_ss(*f64, hop, status=st)
    with pytest.raises(GolfError, match="chunked"):
        GF.ltv_allpole_ss(*f32, hop, mode="fp64", status=st)
    # under autocast every input goes through custom_fwd(cast_inputs=torch.float32) exactly as before: it casts half
    # tensors to fp32 and leaves float64 ones alone, which the fp32 kernels then refuse -- the double path is not taken
    plain = GF.ltv_allpole_ss(*f32, hop)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert torch.equal(GF.ltv_allpole_ss(*f32, hop), plain)
        with pytest.raises(GolfError, match="fp32"):
            GF.ltv_allpole_ss(*f64, hop)


@pytest.mark.parametrize("B,F,M,hop", [(2, 9, 22, 240), (2, 9, 22, 100)])   # on the ring grid, off it
def test_fp32_calls_are_untouched(B, F, M, hop):
    """No hidden shared workspace or flag: an fp32 call without a mode gives the same bits before and after the float64
    recursion ran in the process, forward and gradients."""
    ex, gain, a, gy, T, _ = case(B, F, M, hop, None, 0.5)
    before = run(ex, gain, a, gy, hop, torch.float32)
    run(ex, gain, a, gy, hop, torch.float64)
    run(ex, gain, a, gy, hop, torch.float32, mode="fp64")
    after = run(ex, gain, a, gy, hop, torch.float32)
    for u, v in zip(before, after):
        assert torch.equal(u, v)
