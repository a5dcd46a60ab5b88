"""GPU parity of the fused residual (golf_ltv_residual_f32 / golf_ltv_residual_stream_f32, csrc/lpc_residual.hip;
functional.ltv_residual / ltv_residual_stream, GlottalSourceAnalysis.residual_fused, analysis_stream.ResidualStream) against
the float64 restatement of its definition (tests/residual_ref.py) on the same fp32 inputs.

Bar: the largest error, in units of the case's largest reference magnitude, is at most four times that of the restatement's
fp32 stand-in (the same steps in numpy float32) on the same case -- the project's convention.  The numerator has
golf_ltv_inverse_f32's bits: with a gain of ones the result is ``torch.equal`` to ``ltv_inverse``.  The agreement with
``GlottalSourceAnalysis.residual`` (torch's gain interpolation, whose weight error grows with t) is reported, not asserted.
profiles/residual_parity.txt has the measured figures per case next to the stand-in's.

Largest measured errors over the cases on an MI355X: 8.0e-07 of the case's largest value (hop 5, M 17; the stand-in has the
same 8.0e-07); the largest ratio to the stand-in is 1.28 (hop 300, M 64: 5.3e-07 against 4.1e-07).  Against ``residual()`` the
fused result differs by up to 8.2e-07 on these short cases and by 3.9e-06 at two seconds (profiles/
env_glottal_stream_timing.txt)."""
import numpy as np
import pytest
import torch

import residual_ref as R

pytestmark = pytest.mark.gpu

# (B, F, M, hop, T): the cases of tests/test_gpu_lpc_inverse.py, then F = 1 and an input longer than (F - 1) hop + 1
CASES = [
    (2, 6, 64, 1, 6),
    (2, 9, 33, 3, 25),
    (1, 2, 64, 500, 501),
    (3, 5, 1, 7, 29),
    (2, 7, 40, 16, 70),
    (2, 3, 64, 300, 130),
    (2, 4, 22, 240, 721),
    (2, 12, 17, 5, 56),
    (3, 1, 22, 240, 7),           # F = 1: one sample, e[0] = x[0] / gain[0]
    (2, 4, 30, 12, 56),           # clipped to (F - 1) hop + 1 = 37 samples
    (8, 2, 2, 7, 8),              # one tile per row: the rows tests/test_gpu_grid_folds.py tiles past the grid's fold
]


def dev(a):
    return a if isinstance(a, torch.Tensor) else torch.tensor(a).cuda()


def inputs(case):
    B, F, M, hop, T = case
    return R.inputs(B, F, M, T, seed=100 * M + hop)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_F%d_M%d_hop%d_T%d" % c)
def test_parity_against_the_float64_restatement(case):
    from golf_amd import functional as GF
    from golf_amd.glottal import GlottalSourceAnalysis

    B, F, M, hop, T = case
    x, gain, a = inputs(case)
    ref, stand_in = R.residual(x, gain, a, hop), R.residual(x, gain, a, hop, fp32=True)
    e = GF.ltv_residual(dev(x), dev(gain), dev(a), hop)
    assert e.shape == ref.shape == (B, R.length(T, F, hop)) and e.dtype == torch.float32 and not e.requires_grad
    assert e.is_contiguous() and torch.isfinite(e).all()
    err, bar = R.error(e.cpu().numpy(), ref), 4 * R.error(stand_in, ref)
    # the numerator's bits: a gain of ones divides nothing away
    assert torch.equal(GF.ltv_residual(dev(x), torch.ones_like(dev(gain)), dev(a), hop), GF.ltv_inverse(dev(x), dev(a), hop))
    m = GlottalSourceAnalysis(torch.zeros(2, 8), 24000.0, hop)
    chain = m.residual(dev(x), dev(gain), dev(a))
    assert torch.equal(m.residual_fused(dev(x), dev(gain), dev(a)), e) and chain.shape == e.shape
    print(f"residual B{B} F{F} M{M} hop{hop} T{T}: error {err:.3e}  fp32 stand-in {bar / 4:.3e}  bar {bar:.3e}  "
          f"against residual() (torch's gain interpolation) {R.error(chain.cpu().numpy(), e.cpu().numpy()):.3e}")
    assert err <= bar
    if F == 1:
        assert torch.equal(e[:, 0], dev(x)[:, 0] / dev(gain)[:, 0])


def test_strided_rows_reproducible_and_batch_independent():
    from golf_amd import functional as GF

    B, F, M, hop, T = 3, 5, 40, 16, 60
    x, gain, a = (dev(t) for t in R.inputs(B, F, M, T, 9))
    first = GF.ltv_residual(x, gain, a, hop)
    wide = torch.full((B, T + 37), float("nan"), device="cuda")
    wide[:, 5:5 + T] = x
    view = wide[:, 5:5 + T]
    assert not view.is_contiguous()
    assert torch.equal(GF.ltv_residual(view, gain, a, hop), first)
    assert torch.equal(GF.ltv_residual(x, gain, a, hop), first)
    for b in range(B):
        assert torch.equal(GF.ltv_residual(x[b:b + 1], gain[b:b + 1], a[b:b + 1], hop)[0], first[b])
    assert torch.equal(GF.ltv_residual(x.flip(0), gain.flip(0), a.flip(0), hop).flip(0), first)


def test_graph_capture_replays_the_eager_result():
    from golf_amd import functional as GF

    B, F, M, hop, T = 2, 4, 22, 240, 721
    x, gain, a = (dev(t) for t in R.inputs(B, F, M, T, 5))
    eager = GF.ltv_residual(x, gain, a, hop)
    sx, sg, sa = torch.zeros_like(x), torch.ones_like(gain), torch.zeros_like(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        GF.ltv_residual(sx, sg, sa, hop)   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = GF.ltv_residual(sx, sg, sa, hop)
    sx.copy_(x), sg.copy_(gain), sa.copy_(a)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_autocast_grad_empty_batch_and_refusals():
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError

    B, F, M, hop, T = 2, 6, 22, 16, 81
    x, gain, a = (dev(t) for t in R.inputs(B, F, M, T, 3))
    want = GF.ltv_residual(x.half().float(), gain.half().float(), a.half().float(), hop)
    with torch.autocast("cuda", dtype=torch.float16):
        got = GF.ltv_residual(x.half(), gain.half(), a.half(), hop)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    with pytest.raises(GolfError, match="fp32"):
        GF.ltv_residual(x.half(), gain, a, hop)
    out = GF.ltv_residual(x.clone().requires_grad_(True), gain, a.clone().requires_grad_(True), hop)
    assert not out.requires_grad and torch.equal(out, GF.ltv_residual(x, gain, a, hop))
    empty = GF.ltv_residual(x[:0], gain[:0], a[:0], hop)
    assert empty.shape == (0, 81) and empty.is_cuda and empty.dtype == torch.float32
    assert GF.ltv_residual(x[:, :0], gain, a, hop).shape == (B, 0)
    assert GF.ltv_residual_stream(x, gain, a, 0, 0, 0, 0, False, hop).shape == (B, 0)
    with pytest.raises(GolfError, match="M=65"):   # refused before a launch, on the device too
        GF.ltv_residual(x, gain, torch.zeros(B, F, 65, device="cuda"), hop)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.ltv_residual(x.cpu(), gain.cpu(), a.cpu(), hop)
    zero = GF.ltv_residual(x, torch.zeros_like(gain), a, hop)   # a zero gain gives what IEEE gives
    assert not torch.isfinite(zero).any()


def admissible_windows(T_out, F, M, hop, rng, n=5):
    """Random (t_first, n_out, x_t0, x_end, fr_first, fr_end, last): ``n`` windows without ``last`` where the frames allow
    one, then the utterance's end with ``last``."""
    out = []
    limit = min(T_out, (F - 1) * hop)   # samples whose next frame exists
    for _ in range(n):
        if limit < 1:
            break
        t_first = int(rng.integers(0, limit))
        n_out = int(rng.integers(1, limit - t_first + 1))
        t_end = t_first + n_out
        x_t0 = int(rng.integers(0, max(t_first - M, 0) + 1))
        fr_first = int(rng.integers(0, t_first // hop + 1))
        fr_end = int(rng.integers((t_end - 1) // hop + 2, F + 1))
        out.append((t_first, n_out, x_t0, int(rng.integers(t_end, T_out + 1)), fr_first, fr_end, False))
    t_first = int(rng.integers(0, T_out))
    f_lo = min(t_first // hop, max(F - 2, 0))
    out.append((t_first, T_out - t_first, max(t_first - M, 0), T_out, f_lo, F, True))
    return out


@pytest.mark.parametrize("case", CASES + [(2, 40, 22, 240, 9361), (2, 3, 5, 700, 1401)], ids=lambda c: "B%d_F%d_M%d_hop%d_T%d" % c)
def test_stream_entry_windows_equal_the_one_shot_rows(case):
    from golf_amd import functional as GF

    B, F, M, hop, T = case
    x, gain, a = (dev(t) for t in inputs(case))
    one = GF.ltv_residual(x, gain, a, hop)
    rng = np.random.default_rng(hop + M)
    wins = admissible_windows(one.shape[1], F, M, hop, rng)
    assert wins[-1][-1] and (len(wins) >= 4 or F == 1 or one.shape[1] <= hop)
    for t_first, n_out, x_t0, x_end, fr_first, fr_end, last in wins:
        got = GF.ltv_residual_stream(x[:, x_t0:x_end], gain[:, fr_first:fr_end], a[:, fr_first:fr_end], x_t0, fr_first, t_first,
                                     n_out, last, hop)
        assert torch.equal(got, one[:, t_first:t_first + n_out]), (case, t_first, n_out, x_t0, fr_first, last)
    if one.shape[1] > 3 * hop + M:
        assert any(w[2] > 0 for w in wins) and any(w[4] > 0 for w in wins)


def cuts(n, sizes, rng):
    out = []
    while sum(out) < n:
        out.append(min(int(rng.choice(sizes)), n - sum(out)))
    return out


def stream_run(st, x, gain, a, mode, seed):
    from golf_amd.audiotensor import AudioTensor

    rng = np.random.default_rng(seed)
    hop, M, (T, F) = st.hop, st.order, (x.shape[1], gain.shape[1])
    xs, fs = cuts(T, [0, 1, 1, hop, M + 1, 300, 3 * hop + 1], rng), cuts(F, [0, 1, 2, 3, 10], rng)
    ev = [("x", n) for n in xs] + [("f", n) for n in fs]
    if mode == "mixed":
        ev = [ev[i] for i in rng.permutation(len(ev))]
    elif mode == "frames first":
        ev = [("f", F)] + ev[:len(xs)]
    elif mode == "audio first":
        ev = [("x", T)] + ev[len(xs):]
    outs, px, pf = [], 0, 0
    for kind, n in ev:
        if kind == "x":
            outs.append(st.push(x=AudioTensor(x[:, px:px + n])))
            px += n
        else:
            outs.append(st.push(gain=AudioTensor(gain[:, pf:pf + n], hop), a=a[:, pf:pf + n]))
            pf += n
    assert px == T and pf == F
    outs.append(st.finish())
    assert any(o.shape[1] == 0 for o in outs)
    return torch.cat(outs, 1)


# hop 1 with M 64; hop 3 with M 33; the recipe; a hop above the tile width of 256
@pytest.mark.parametrize("hop,M,F,T", [(1, 64, 700, 650), (3, 33, 200, 640), (240, 22, 13, 3000), (300, 9, 9, 2401)])
def test_stream_equals_the_one_shot(hop, M, F, T):
    from golf_amd import functional as GF
    from golf_amd.analysis_stream import ResidualStream

    x, gain, a = (dev(t) for t in R.inputs(2, F, M, T, hop + M))
    one = GF.ltv_residual(x, gain, a, hop)
    assert one.shape[1] == min(T, (F - 1) * hop + 1) and one.shape[1] > 256
    st = ResidualStream(hop, M, 2)
    for mode, seed in (("mixed", 1), ("mixed", 2), ("frames first", 3), ("audio first", 4)):
        got = stream_run(st, x, gain, a, mode, seed)
        assert got.is_cuda and got.dtype == torch.float32 and torch.equal(got, one), (mode, seed)
    alone = stream_run(ResidualStream(hop, M, 1), x[1:], gain[1:], a[1:], "mixed", 5)
    assert torch.equal(alone[0], one[1])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h = st.push(x.bfloat16(), gain.bfloat16(), a.bfloat16())
        h = torch.cat([h, st.finish()], 1)
    assert torch.equal(h, GF.ltv_residual(x.bfloat16().float(), gain.bfloat16().float(), a.bfloat16().float(), hop))
