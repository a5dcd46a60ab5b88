"""The plain side of the frame-wise all-pole filter's tests (csrc/lpc_ff.hip): which kernel a shape takes, the table of cases
that puts every kernel instance under test, their inputs, an fp32 emulation of the plain algorithm and a handful of wrong
oracles.  No GPU: tests/test_ff_ref_host.py checks this file, tests/test_gpu_ff_rings.py runs the kernels on its cases.

The reference stays the float64 oracle (oracle.golf_oracle.lti_frames_ola_forward / _backward).

Inputs (``inputs``): excitation N(0,1); an INDEPENDENT coefficient row per frame -- reflection-coefficient logits N(0, scale)
per (b, f) through rc2lpc(tanh(.)) -- and an independent gain exp(N(-3, 0.5)) per frame, so that a kernel reading row f +- 1
or gain segment s +- 1 is far off, not close to the bar as on a 0.02 random walk; Hann window; cotangent
default_rng(1).normal.  scale 0.5 up to M = 22, 0.25 above (at 0.5 with M = 38 and W = 160 a sequential fp32 direct form is
itself at 6e-5)."""
from collections import namedtuple

import numpy as np

TOL_Y, TOL_G = 1e-4, 2e-4          # the bars of tests/test_gpu_lpc_ff_anyshape.py, rel-max and rel-l2
OUTPUTS = ("y", "g_ex", "g_gain", "g_a")
BARS = dict(y=TOL_Y, g_ex=TOL_G, g_gain=TOL_G, g_a=TOL_G)
RINGS = ((8, 6), (16, 14), (24, 22), (32, 30), (40, 38))   # (ring, taps) of the five template instances
KAPPA = 64.0                       # GOLF_FF_KAPPA


# ---- routing: golf_lti_frames_ola_{fwd,bwd}_f32 and golf_lti_frames_ola_stream_f32 restated ------------------------------
def _block_ok(taps, hop, W):
    return taps <= 24 and W % 32 == 0 and hop % 4 == 0 and 4 * (3 * hop + W) <= 56 * 1024


def route(M, hop, W):
    """(forward, backward) kernel labels of the one-shot entries."""
    pick = next(((ring, taps) for ring, taps in RINGS if M <= taps and ring <= hop), None)
    if pick is None:
        return "any", "any"
    ring, taps = pick
    fwd = f"block<{taps}>" if _block_ok(taps, hop, W) else f"{'quad' if W % ring == 0 else 'scalar'}<{ring},{taps}>"
    bwd = f"ring<{ring},{taps}>" if W % ring == 0 and 16 * (2 * W + ring + 6) <= 64 * 1024 else "any"
    return fwd, bwd


def stream_route(M, hop, W):
    """Kernel label of the stream entry (M <= 38): the block recursion where the one-shot entry takes it, else the scalar
    kernel of the order's class, whatever the hop."""
    pick = next((taps for ring, taps in RINGS if M <= taps and ring <= hop), None)
    if pick is not None and _block_ok(pick, hop, W):
        return f"block<{pick}>"
    return f"scalar<{next(taps for _, taps in RINGS if M <= taps)}>"


def kappa(a_row, NT=None):
    """The block-recursion kernels' conditioning number of one coefficient row, in float64: the largest row sum of |G|,
    G[s] = e_0^T C^(s+1), s = 0 .. 15, from the recurrence v <- (v[1:] - a[:-1] v0, -a[-1] v0) started at e_0."""
    a = np.zeros(NT or len(a_row))
    a[:len(a_row)] = a_row
    v = np.zeros(len(a))
    v[0] = 1.0
    worst = 0.0
    for _ in range(16):
        v0 = v[0]
        v = np.append(v[1:] - a[:-1] * v0, -a[-1] * v0)
        worst = max(worst, np.abs(v).sum())
    return worst


# ---- the table ---------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "M hop W B F Tx fwd bwd stream")

# (B, F) per forward kernel: around 16 frames per wave (quad), 4 per wave (block), 64 (b, f) per block (scalar); each set has
# B*F % 4 != 0 (ff_grad_a_kernel and the wave-per-frame g_a take four (b, f) per block)
QUAD_BF = ((1, 15), (2, 16), (3, 17), (1, 33))
BLOCK_BF = ((3, 3), (2, 4), (1, 5), (2, 9))
SCALAR_BF = ((3, 21), (2, 32), (5, 13))

#  (M, hop, W)     forward         backward        stream
ROWS = [
    ((1, 8, 32), "block<6>", "ring<8,6>", "block<6>"),
    ((6, 8, 32), "block<6>", "ring<8,6>", "block<6>"),
    ((7, 16, 32), "block<14>", "ring<16,14>", "block<14>"),
    ((14, 16, 32), "block<14>", "ring<16,14>", "block<14>"),
    ((15, 24, 96), "block<22>", "ring<24,22>", "block<22>"),
    ((22, 24, 96), "block<22>", "ring<24,22>", "block<22>"),
    ((22, 24, 64), "block<22>", "any", "block<22>"),               # ring forward, 64 % 24 != 0
    ((6, 9, 24), "quad<8,6>", "ring<8,6>", "scalar<6>"),
    ((6, 8, 40), "quad<8,6>", "ring<8,6>", "scalar<6>"),           # W = 5 hop: the looped branch of the overlap-add kernels
    ((6, 260, 520), "quad<8,6>", "ring<8,6>", "scalar<6>"),        # hop > 256: ff_bwd_ola_kernel's strided sample loop
    ((14, 18, 48), "quad<16,14>", "ring<16,14>", "scalar<14>"),
    ((22, 24, 72), "quad<24,22>", "ring<24,22>", "scalar<22>"),
    ((23, 32, 64), "quad<32,30>", "ring<32,30>", "scalar<30>"),
    ((30, 32, 64), "quad<32,30>", "ring<32,30>", "scalar<30>"),
    ((31, 40, 80), "quad<40,38>", "ring<40,38>", "scalar<38>"),
    ((38, 40, 80), "quad<40,38>", "ring<40,38>", "scalar<38>"),
    ((38, 40, 160), "quad<40,38>", "ring<40,38>", "scalar<38>"),
    ((6, 8, 18), "scalar<8,6>", "any", "scalar<6>"),
    ((14, 16, 34), "scalar<16,14>", "any", "scalar<14>"),
    ((22, 24, 50), "scalar<24,22>", "any", "scalar<22>"),
    ((30, 32, 66), "scalar<32,30>", "any", "scalar<30>"),
    ((38, 40, 82), "scalar<40,38>", "any", "scalar<38>"),
    ((35, 44, 100), "scalar<40,38>", "any", "scalar<38>"),
]


def tile_counts(fwd):
    return BLOCK_BF if fwd.startswith("block") else QUAD_BF if fwd.startswith("quad") else SCALAR_BF


CASES = [Case(*shape, B, F, None, fwd, bwd, stream) for shape, fwd, bwd, stream in ROWS for B, F in tile_counts(fwd)]
# the hop-260 row at one frame count: its point is the sample loop of one block, not the frame tile
CASES = [c for c in CASES if c.hop != 260 or c.F == 17]


def first_case(fwd=None, bwd=None, shape=None):
    """The first table case with these labels (or this (M, hop, W))."""
    return next(c for c in CASES if (fwd is None or c.fwd == fwd) and (bwd is None or c.bwd == bwd)
                and (shape is None or (c.M, c.hop, c.W) == shape))


def case_id(c):
    tx = "" if c.Tx is None else f"-Tx{c.Tx}"
    return f"M{c.M}-hop{c.hop}-W{c.W}-B{c.B}-F{c.F}{tx}-{c.fwd}-{c.bwd}"


def scale_of(M):
    return 0.5 if M <= 22 else 0.25


def geometry(c):
    """(Tx0, Tx, nfr, Ty): the excitation's length, the part the filter reads, the frames and the output length."""
    Tx0 = (c.F - 1) * c.hop + 1 if c.Tx is None else c.Tx
    Tx = min(Tx0, (c.F - 1) * c.hop + 1)
    pad = c.W // 2
    nfr = (Tx + 2 * pad - c.W) // c.hop + 1
    return Tx0, Tx, nfr, (nfr - 1) * c.hop + c.W - 2 * pad


def hann(W):
    import torch

    return torch.hann_window(W).double().numpy()


_inputs, _refs = {}, {}


def _frozen(*arrays):
    for v in arrays:
        v.setflags(write=False)
    return arrays


def draw_rows(rng, shape, M, scale):
    from oracle import golf_oracle as O

    return O.rc2lpc(np.tanh(rng.normal(0, scale, tuple(shape) + (M,)))).astype(np.float32)


def inputs(c, a=None):
    """(ex, gain, a, window, gy) of a case: fp32 arrays (the window float64), read-only, made once.  ``a``: planted rows
    (B, F, M) in place of the drawn ones (not cached)."""
    if a is None and c in _inputs:
        return _inputs[c]
    Tx0, _, _, Ty = geometry(c)
    rng = np.random.default_rng([c.M, c.hop, c.W, c.B, c.F, Tx0])
    ex = rng.normal(0, 1, (c.B, Tx0)).astype(np.float32)
    rows = draw_rows(rng, (c.B, c.F), c.M, scale_of(c.M))
    gain = np.exp(rng.normal(-3, 0.5, (c.B, c.F))).astype(np.float32)
    gy = np.random.default_rng(1).normal(0, 1, (c.B, Ty)).astype(np.float32)
    out = _frozen(ex, gain, rows if a is None else np.array(a, dtype=np.float32), hann(c.W), gy)
    if a is None:
        _inputs[c] = out
    return out


def oracle(ex, gain, a, win, gy, hop):
    from oracle import golf_oracle as O

    y, _ = O.lti_frames_ola_forward(ex, gain, a, hop, win)
    return dict(zip(OUTPUTS, (y,) + tuple(O.lti_frames_ola_backward(gy, ex, gain, a, hop, win))))


def refs(c, a=None):
    """The oracle's y, g_ex, g_gain, g_a of a case (float64, read-only, computed once)."""
    if a is None and c in _refs:
        return _refs[c]
    ex, gain, rows, win, gy = inputs(c, a)
    out = oracle(ex, gain, rows, win, gy, c.hop)
    _frozen(*out.values())
    if a is None:
        _refs[c] = out
    return out


def distances(got, want):
    """{output: (rel-max, rel-l2)} as conftest.rel_err measures them."""
    from conftest import rel_err

    return {k: rel_err(got[k], want[k]) for k in OUTPUTS}


# ---- the plain algorithm in fp32 ---------------------------------------------------------------------------------------
def emulate_fp32(c, a=None):
    """The plain algorithm in numpy float32 -- a sequential direct-form recursion per frame, fp32 overlap-add, fp32
    correlation sums for g_a -- on the case's inputs: what any fp32 implementation may be expected to reach."""
    f32 = np.float32
    ex, gain, rows, win, gy = inputs(c, a)
    win = win.astype(f32)
    M, hop, W, B, F = c.M, c.hop, c.W, c.B, c.F
    _, Tx, nfr, Ty = geometry(c)
    pad = W // 2
    t = np.arange(Tx)
    seg = np.minimum(t // hop, F - 2)
    G = gain[:, seg] + (t - seg * hop).astype(f32) * ((gain[:, seg + 1] - gain[:, seg]) * f32(1.0 / hop))
    xp = np.zeros((B, Tx + 2 * pad), f32)
    xp[:, pad:pad + Tx] = ex[:, :Tx] * G
    idx = np.arange(nfr)[:, None] * hop + np.arange(W)[None]

    def recursion(x, reverse):      # x (B, nfr, W); the all-pole recursion per frame, term by term in fp32
        x = x[..., ::-1] if reverse else x
        yp = np.zeros((B, nfr, W + M), f32)
        for k in range(W):
            acc = x[..., k].copy()
            for i in range(M):
                acc -= rows[:, :nfr, i] * yp[..., M + k - 1 - i]
            yp[..., M + k] = acc
        return yp[..., :M - 1:-1] if reverse else yp[..., M:]

    def ola(fr):                    # (B, nfr, W) -> (B, full), frame by frame in fp32
        acc = np.zeros((B, (nfr - 1) * hop + W), f32)
        for f in range(nfr):
            acc[:, f * hop:f * hop + W] += fr[:, f]
        return acc

    yf = recursion(xp[:, idx], False)
    norm = ola(np.broadcast_to(win, (1, nfr, W)))[0, pad:pad + Ty]
    y = ola(yf * win)[:, pad:pad + Ty] / norm
    gq = np.zeros((B, (nfr - 1) * hop + W), f32)
    gq[:, pad:pad + Ty] = gy / norm
    u = recursion(gq[:, idx] * win, True)
    g_a = np.zeros((B, F, M), f32)
    ypad = np.concatenate([np.zeros((B, nfr, M), f32), yf], 2)
    for i in range(M):
        prod = u * ypad[..., M - 1 - i:M - 1 - i + W]
        acc = np.zeros((B, nfr), f32)
        for k in range(W):          # the correlation sum, term by term
            acc += prod[..., k]
        g_a[:, :nfr, i] = -acc
    g_x = ola(u)[:, pad:pad + Tx]
    g_ex = np.zeros(ex.shape, f32)
    g_ex[:, :Tx] = g_x * G
    w = (t - seg * hop).astype(f32) * f32(1.0 / hop)
    gG = g_x * ex[:, :Tx]
    g_gain = np.zeros((B, F), f32)
    for s in range(F - 1):          # hat-weighted sums per gain segment
        m = seg == s
        g_gain[:, s] += ((f32(1) - w[m]) * gG[:, m]).sum(1, dtype=f32)
        g_gain[:, s + 1] += (w[m] * gG[:, m]).sum(1, dtype=f32)
    return dict(y=y, g_ex=g_ex, g_gain=g_gain, g_a=g_a)


# ---- wrong oracles -----------------------------------------------------------------------------------------------------
def _shifted(v):                    # row f+1 in place of row f (the last row stays)
    return np.concatenate([v[:, 1:], v[:, -1:]], 1)


def _mut_next_row(c):
    ex, gain, a, win, gy = inputs(c)
    return oracle(ex, gain, _shifted(a), win, gy, c.hop)


def _mut_gain_shift(c):
    ex, gain, a, win, gy = inputs(c)
    out = oracle(ex, _shifted(gain), a, win, gy, c.hop)
    out["g_gain"] = _shifted(refs(c)["g_gain"])     # g_x does not depend on the gain: the wrong segment on the way out
    return out


def _mut_last_tap(c):
    ex, gain, a, win, gy = inputs(c)
    a = a.copy()
    a[..., -1] = 0
    return oracle(ex, gain, a, win, gy, c.hop)


def _mut_norm_index(c):
    """The normaliser summed over window[k + 1] (window[W] = 0): y and g_q scale by norm / norm'."""
    ex, gain, a, win, gy = inputs(c)
    _, _, nfr, Ty = geometry(c)
    norm, wrong = np.zeros((2, (nfr - 1) * c.hop + c.W))
    for f in range(nfr):
        norm[f * c.hop:f * c.hop + c.W] += win
        wrong[f * c.hop:f * c.hop + c.W - 1] += win[1:]
    ratio = norm[c.W // 2:c.W // 2 + Ty] / wrong[c.W // 2:c.W // 2 + Ty]
    out = oracle(ex, gain, a, win, gy * ratio, c.hop)
    out["y"] = refs(c)["y"] * ratio
    return out


def _mut_unused_rows(c):
    """g_a of the frames f >= nfr: the last used frame's instead of zero."""
    out = dict(refs(c))
    nfr = geometry(c)[2]
    out["g_a"] = out["g_a"].copy()
    out["g_a"][:, nfr:] = out["g_a"][:, nfr - 1:nfr]
    return out


def _mut_drop_last_frame(c):
    """The last frame left out of the forward's overlap-add and of every gradient: the oracle on the excitation one hop
    shorter, zero-extended."""
    ex, gain, a, win, gy = inputs(c)
    _, Tx, nfr, Ty = geometry(c)
    short = oracle(ex[:, :Tx - c.hop], gain, a, win, gy[:, :Ty - c.hop], c.hop)
    out = {k: np.zeros_like(v) for k, v in refs(c).items()}
    out["y"][:, :Ty - c.hop] = short["y"]
    out["g_ex"][:, :Tx - c.hop] = short["g_ex"]
    out["g_gain"], out["g_a"] = short["g_gain"], short["g_a"]
    return out


Mutant = namedtuple("Mutant", "make outputs meant_for")
MUTANTS = {
    "coefficient row f+1": Mutant(_mut_next_row, OUTPUTS, lambda c: True),
    "gain segment s+1": Mutant(_mut_gain_shift, OUTPUTS, lambda c: True),
    "last tap dropped": Mutant(_mut_last_tap, OUTPUTS, lambda c: True),
    # a Hann window of a whole number of hops sums to a constant, whichever index, wherever all its frames exist (every sample
    # at two hops): the cases that can tell are those of other windows and those that are mostly the utterance's two ends
    # (y and g_ex carry it sample by sample; g_gain and g_a are sums over a frame, in which it partly averages out)
    "normaliser index + 1": Mutant(_mut_norm_index, ("y", "g_ex"),
                                   lambda c: c.W % c.hop != 0 or (c.W != 2 * c.hop and c.F * c.hop <= 2 * c.W)),
    "g_a past nfr": Mutant(_mut_unused_rows, ("g_a",), lambda c: geometry(c)[2] < c.F),
    "last frame omitted": Mutant(_mut_drop_last_frame, OUTPUTS, lambda c: True),
}


# ---- ragged variants and planted conditioning tiers ---------------------------------------------------------------------
def ragged(c):
    """{name: case}: the excitation ending inside the last frame, two frames short (nfr < F), and running on past
    (F-1)*hop + 1."""
    end = (c.F - 1) * c.hop + 1
    return dict(inside=c._replace(Tx=end - 1 - c.hop // 3), short=c._replace(Tx=end - 2 * c.hop), long=c._replace(Tx=end + 37))


# one row per forward kernel; between them both backward chains
RAGGED_ROWS = [first_case("block<14>", "ring<16,14>", (14, 16, 32))._replace(B=2, F=9),
               first_case("block<22>", "any")._replace(B=2, F=9),
               first_case("quad<40,38>", "ring<40,38>", (38, 40, 80))._replace(B=2, F=17),
               first_case("scalar<24,22>", "any")]

TIER_SHAPES = ((14, 16, 64), (22, 24, 96))
LOW, HIGH = 16.0, 256.0            # a factor four clear of GOLF_FF_KAPPA = 64 on both sides
HIGH_FRAMES = (5, 8, 9, 10, 11)    # wave 0 all low; wave 1 one high frame; wave 2 all high
SWAPPED = 5
_planted = {}


def span(c, f):
    """The output samples frame f reaches."""
    lo = f * c.hop - c.W // 2
    return slice(max(lo, 0), min(lo + c.W, geometry(c)[3]))


def span_distances(c, y, ref):
    """(rel-max, rel-l2) of y on each frame's own span: every frame on its own scale."""
    from conftest import rel_err

    return [rel_err(y[:, span(c, f)], ref[:, span(c, f)]) for f in range(geometry(c)[2])]


def planted(shape):
    """(case, a, a_low, kappas) of the tier test: one utterance of 12 frames whose rows are SELECTED, not assumed -- frames
    0..4, 6, 7 with kappa <= 16, frames 5 and 8..11 with kappa >= 256, and among such draws the first (seeded) utterance on
    which the plain fp32 algorithm stays within a third of every bar.  ``a_low``: the same with frame 5 replaced by a low
    row."""
    if shape in _planted:
        return _planted[shape]
    M, hop, W = shape
    fwd, bwd = route(M, hop, W)
    c = Case(M, hop, W, 1, 12, None, fwd, bwd, stream_route(M, hop, W))
    NT = int(fwd[6:-1])
    rng = np.random.default_rng([M, hop, W, 7])

    def pool(scale, ok, n):
        got = []
        while len(got) < n:
            for row in draw_rows(rng, (64,), M, scale):
                if ok(kappa(row, NT)):
                    got.append(row)
        return got[:n]

    for _ in range(200):
        low, high = pool(0.25, lambda k: k <= LOW, c.F + 1), pool(1.0, lambda k: HIGH <= k <= 4096.0, len(HIGH_FRAMES))
        a = np.stack([high.pop() if f in HIGH_FRAMES else low.pop() for f in range(c.F)])[None]
        want, got = refs(c, a), emulate_fp32(c, a)
        if all(max(d) <= BARS[k] / 3 for k, d in distances(got, want).items()) and \
                max(max(d) for d in span_distances(c, got["y"], want["y"])) <= TOL_Y / 3:
            a_low = a.copy()
            a_low[0, SWAPPED] = low.pop()
            kappas = [kappa(r, NT) for r in a[0]] + [kappa(a_low[0, SWAPPED], NT)]
            _planted[shape] = (c, a, a_low, kappas)
            return _planted[shape]
    raise AssertionError(f"no planted utterance for {shape} within a third of the bars in 200 draws")


# ---- stream rows: one per stream kernel ---------------------------------------------------------------------------------
# scalar: 70 frames in one call (more than the 64 of a block); block recursion: 9 and 10 frames (4 per wave)
STREAM_CASES = [Case(*shape, B, F, None, fwd, bwd, stream)
                for shape, B, F in (((6, 8, 32), 2, 9), ((14, 16, 32), 2, 10), ((22, 24, 96), 2, 9), ((6, 9, 24), 2, 70),
                                    ((14, 18, 48), 1, 70), ((22, 24, 72), 2, 70), ((30, 32, 64), 1, 70), ((38, 40, 80), 2, 70))
                for fwd, bwd in (route(*shape),) for stream in (stream_route(*shape),)]
