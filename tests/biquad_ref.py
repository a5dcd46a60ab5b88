"""Cases and yardsticks for the cascaded-biquad frame filter (TEST INFRASTRUCTURE; numpy and torch on the CPU).

The operation (oracle.golf_oracle.biquad_frames_ola_forward, reference models/lpc.py:94-131): zero-pad the excitation by
``pad``, cut frames of W every hop, run frame f through its K sections 1/(a0 + a1 z^-1 + a2 z^-2) from a zero state, window,
overlap-add, divide by the overlap-add of the window.  Two conventions, the ones golf_amd.functional.biquad_frames_ola
documents:
    frame_gain=True,  pad = (W-hop)//2   frame f as a whole is scaled by gain[b, f]        (BatchSecondOrderLPCSynth)
    frame_gain=False, pad = W//2         the excitation is scaled by the gain interpolated to sample rate before framing;
                                         only its first (F-1)*hop + 1 samples are used       (LTVMinimumPhaseFilter)

    make_case          float32 inputs of a shape in either convention, sections with a0 != 1
    cascade_f32        the oracle's algorithm in sequential float32: what ANY fp32 cascade loses on an input
    torch_cascade_f64  pad / unfold / K explicit recursions / window / fold / normalise in float64 torch, gradients by
                       autograd: a second yardstick for the oracle's closed-form backward

FRAME_GAIN_SHAPES / INTERP_GAIN_SHAPES / HARSH_SHAPES are the shapes tests/test_gpu_biquad_cascade.py runs on the GPU and
tests/test_biquad_ref_host.py checks the yardsticks on.  Every id names the boundary of the kernel the shape is there for
(csrc/lpc_ff.hip: 16 lanes per frame, 4 frames per wave, W + K - 1 pipeline steps in pairs of 4-step blocks, the wave's
frames staged as one union of XS = 3*hop + W + 40 floats in strides of 512).  blocks = ceil((W + K - 1) / 4): the
``q += 2`` loop runs its second block only while q + 1 < blocks, so an odd count ends on a lone first block."""
import numpy as np
import torch

# id: (B, K, hop, W, nfr, extra_F, ragged); F = nfr + extra_F, the excitation has (nfr-1)*hop + W - 2*pad + ragged samples
FRAME_GAIN_SHAPES = {
    "K1-one-frame-W8-blocks2": (2, 1, 4, 8, 1, 0, 0),              # first lane = last lane; nfr = 1; smallest XS (60)
    "K2-nfr2-extraF-ragged-blocks9": (2, 2, 8, 32, 2, 1, 3),       # odd block count; one zeroed gradient row
    "K3-nfr3-W50-blocks13": (3, 3, 16, 50, 3, 0, 5),               # W % 4 = 2, W < 64, W % hop != 0, odd blocks
    "K4-full-wave-W96-blocks25": (1, 4, 24, 96, 4, 2, 0),          # nfr % 4 = 0, 64 < W < 128, two zeroed rows
    "K8-nfr5-W30-blocks10": (2, 8, 8, 30, 5, 0, 1),                # two waves, the second with one frame; W % 4 = 2
    "K11-nfr7-W160-blocks43": (2, 11, 40, 160, 7, 0, 0),           # second wave with three frames; odd blocks
    "K15-nfr9-W64-blocks20": (1, 15, 16, 64, 9, 3, 7),             # W = 64 exactly; three waves; even blocks
    "K16-whole-row-W200-blocks54": (2, 16, 64, 200, 6, 0, 0),      # lane 15 writes; W % 64 = 8; second wave of two
    "K16-W904-XS1664-bwd-lds-65376": (2, 16, 240, 904, 4, 0, 0),   # four staging strides; backward 160 bytes under its limit
    # added to the issue's table:
    "K6-W2hop-unused-tail": (2, 6, 16, 32, 3, 1, 13),              # ragged > pad: 5 excitation samples reach no frame
    "K5-W448-XS536-blocks113": (1, 5, 16, 448, 2, 0, 0),           # 24 floats into the second staging stride
}

# id: (B, K, hop, W, F, extra_F, ragged); nfr = F - extra_F, the excitation has (nfr-1)*hop + 1 + ragged samples
INTERP_GAIN_SHAPES = {
    "K1-F2-W8": (2, 1, 4, 8, 2, 0, 0),                             # the smallest legal interpolated case
    "K5-F4-W32-blocks9": (2, 5, 8, 32, 4, 0, 0),                   # one full wave, odd blocks
    "K16-F5-W48": (3, 16, 16, 48, 5, 0, 0),                        # whole row, a second wave of one frame
    "K12-F8-W480-XS880": (1, 12, 120, 480, 8, 0, 0),               # XS between one and two staging strides
    "K7-F15-W100": (2, 7, 24, 100, 15, 0, 0),                      # W % 64 = 36, four waves, the last with three
    # added to the issue's list:
    "K3-F4-W16-excitation-past-the-gain": (2, 3, 8, 16, 4, 0, 5),  # 5 samples past (F-1)*hop + 1: unused, zero gradient
    "K3-F6-nfr4-W16-extraF": (2, 3, 8, 16, 6, 2, 5),               # F > nfr with an interpolated gain
}

# the conditioning test: sigma = 1.0, max_pole = 0.99, per-frame gain; columns as FRAME_GAIN_SHAPES
HARSH_SHAPES = {
    "harsh-K16-W200": (2, 16, 64, 200, 6, 0, 0),
    "harsh-K14-W960": (2, 14, 240, 960, 5, 0, 0),                  # the largest K whose backward fits W = 960
}


def make_case(B, K, hop, W, nfr, extra_F, ragged, frame_gain, seed, sigma=0.7, max_pole=0.95):
    """float32 ``ex (B,Tx), gain (B,F), biquads (B,F,K,3), window (W,), pad`` with F = nfr + extra_F coefficient frames and
    an excitation that makes exactly nfr frames with ``ragged`` (< hop) samples to spare.  Sections from
    get_logits2biquads("coef", max_pole) on N(0, sigma) logits, each then scaled by its own a0 in [0.8, 1.25]."""
    from golf_amd.utils import get_logits2biquads

    assert 0 <= ragged < hop and nfr >= 1 and extra_F >= 0
    rng = np.random.default_rng(seed)
    F = nfr + extra_F
    pad = (W - hop) // 2 if frame_gain else W // 2
    Tx = (nfr - 1) * hop + W - 2 * pad + ragged if frame_gain else (nfr - 1) * hop + 1 + ragged
    # formed in float64 and rounded once: the float32 inputs, and with them every error figure, are the same on any host
    logits = torch.from_numpy(rng.normal(0, sigma, (B, F, K, 2)))
    bq = get_logits2biquads("coef", max_pole)(logits).numpy()
    bq = (bq * rng.uniform(0.8, 1.25, (B, F, K, 1))).astype(np.float32)
    gain = np.exp(rng.normal(-1, 0.3, (B, F))).astype(np.float32)
    ex = rng.normal(0, 1, (B, Tx)).astype(np.float32)
    window = torch.hann_window(W).numpy()
    return ex, gain, bq, window, pad


def _geometry(Tx, F, hop, W, pad, frame_gain):
    T = Tx if frame_gain else min(Tx, (F - 1) * hop + 1)
    nfr = (T + 2 * pad - W) // hop + 1
    assert 1 <= nfr <= F, (nfr, F)
    return T, nfr


def cascade_f32(ex, gain, biquads, hop, window, pad=None, frame_gain=True):
    """oracle.golf_oracle.biquad_frames_ola_forward with every operation in float32, one sample after the other (all
    frames at once: they do not depend on each other).  Returns a float32 (B, Ty) array."""
    f32 = np.float32
    ex, gain, bq, window = (np.asarray(v, dtype=f32) for v in (ex, gain, biquads, window))
    W = window.shape[0]
    pad = (W - hop) // 2 if pad is None else pad
    B, F = gain.shape
    T, nfr = _geometry(ex.shape[1], F, hop, W, pad, frame_gain)
    if frame_gain:
        x = ex
    else:
        n = np.arange(T)
        f = np.minimum(n // hop, F - 2)
        w = ((n - f * hop) / f32(hop)).astype(f32)
        x = ex[:, :T] * (gain[:, f] * (f32(1) - w) + gain[:, f + 1] * w)
    xp = np.pad(x, ((0, 0), (pad, pad)))
    idx = np.arange(nfr)[:, None] * hop + np.arange(W)[None, :]
    v = xp[:, idx]                                                   # (B, nfr, W)
    if frame_gain:
        v = v * gain[:, :nfr, None]
    for k in range(bq.shape[2]):
        a0, a1, a2 = (bq[:, :nfr, k, i] for i in range(3))
        y = np.zeros((B, nfr, W + 2), dtype=f32)
        for n in range(W):
            y[:, :, n + 2] = (v[:, :, n] - a1 * y[:, :, n + 1] - a2 * y[:, :, n]) / a0
        v = y[:, :, 2:]
    assert v.dtype == f32
    full = (nfr - 1) * hop + W
    acc = np.zeros((B, full), dtype=f32)
    norm = np.zeros(full, dtype=f32)
    for f in range(nfr):
        acc[:, f * hop: f * hop + W] += v[:, f] * window
        norm[f * hop: f * hop + W] += window
    return acc[:, pad: full - pad] / norm[pad: full - pad]


def torch_cascade_f64(ex, gain, biquads, hop, window, pad=None, frame_gain=True, gy=None):
    """numpy in, numpy out, float64 torch in between: ``y`` or, with ``gy``, ``(y, g_ex, g_gain, g_biquads)`` of
    sum(y * gy) by autograd."""
    grad = gy is not None
    x0, g, bq = (torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=grad) for v in (ex, gain, biquads))
    win = torch.as_tensor(np.asarray(window, dtype=np.float64))
    W = win.numel()
    pad = (W - hop) // 2 if pad is None else pad
    B, F = g.shape
    T, nfr = _geometry(x0.shape[1], F, hop, W, pad, frame_gain)
    if frame_gain:
        x = x0
    else:
        n = torch.arange(T)
        f = torch.clamp(n // hop, max=F - 2)
        w = (n - f * hop).double() / hop
        x = x0[:, :T] * (g[:, f] * (1 - w) + g[:, f + 1] * w)
    xp = torch.nn.functional.pad(x, (pad, pad))
    v = xp.unfold(1, W, hop)                                         # (B, nfr', W), nfr' == nfr
    assert v.shape[1] == nfr
    if frame_gain:
        v = v * g[:, :nfr, None]
    for k in range(bq.shape[2]):
        a0, a1, a2 = (bq[:, :nfr, k, i] for i in range(3))
        y1 = y2 = torch.zeros(B, nfr, dtype=torch.float64)
        out = []
        for n in range(W):
            yn = (v[:, :, n] - a1 * y1 - a2 * y2) / a0
            out.append(yn)
            y1, y2 = yn, y1
        v = torch.stack(out, dim=2)
    full = (nfr - 1) * hop + W
    fold = lambda fr: torch.nn.functional.fold(fr.transpose(1, 2), (1, full), (1, W), stride=(1, hop)).reshape(-1, full)
    acc = fold(v * win)
    norm = fold(win.expand(1, nfr, W))
    y = acc[:, pad: full - pad] / norm[:, pad: full - pad]
    if not grad:
        return y.detach().numpy()
    (y * torch.as_tensor(np.asarray(gy, dtype=np.float64))).sum().backward()
    return y.detach().numpy(), x0.grad.numpy(), g.grad.numpy(), bq.grad.numpy()


# ---- the cases themselves: one fixed seed per id (tests/test_biquad_ref_host.py holds each to its fp32 condition) -----------
CASES = {}
for _i, (_cid, _s) in enumerate(FRAME_GAIN_SHAPES.items()):
    CASES[_cid] = dict(shape=_s, frame_gain=True, seed=1000 + _i)
for _i, (_cid, (_B, _K, _hop, _W, _F, _xF, _rag)) in enumerate(INTERP_GAIN_SHAPES.items()):
    CASES[_cid] = dict(shape=(_B, _K, _hop, _W, _F - _xF, _xF, _rag), frame_gain=False, seed=2000 + _i)
# these inputs are heavy-tailed: of seeds 3000..3011 the sequential fp32 cascade loses 1.5e-6 .. 5.6e-3 at K = 16 and
# 2.6e-6 .. 5.8e-2 at K = 14.  The seeds kept are the hardest of those twelve under the cap of 1e-3 with a factor 2 to spare:
# 4.4e-4 at K = 16 and 6.2e-5 at K = 14 (the next one up there is 8.9e-4)
for _cid, _seed in zip(HARSH_SHAPES, (3003, 3011)):
    CASES[_cid] = dict(shape=HARSH_SHAPES[_cid], frame_gain=True, seed=_seed, sigma=1.0, max_pole=0.99)

_cache = {}


def case(cid):
    """The inputs and geometry of case ``cid`` as a dict (built once; treat the arrays as read-only).  ``used`` is the number
    of leading excitation samples that reach a frame, ``Ty`` the output length."""
    if cid not in _cache:
        spec = CASES[cid]
        B, K, hop, W, nfr, extra_F, ragged = spec["shape"]
        fg = spec["frame_gain"]
        kw = {k: spec[k] for k in ("sigma", "max_pole") if k in spec}
        ex, gain, bq, win, pad = make_case(B, K, hop, W, nfr, extra_F, ragged, fg, spec["seed"], **kw)
        F, Tx = nfr + extra_F, ex.shape[1]
        T, nfr_ = _geometry(Tx, F, hop, W, pad, fg)
        assert nfr_ == nfr
        for v in (ex, gain, bq, win):
            v.setflags(write=False)
        _cache[cid] = dict(ex=ex, gain=gain, bq=bq, win=win, pad=pad, hop=hop, frame_gain=fg, seed=spec["seed"], B=B, K=K,
                           W=W, F=F, nfr=nfr, Tx=Tx, used=min(T, (nfr - 1) * hop + W - pad),
                           Ty=(nfr - 1) * hop + W - 2 * pad)
    return _cache[cid]


def make_gy(ref, seed):
    """A random output gradient scaled by 1 / max|ref| (float32): the loss sum(y * gy) is then O(1) per sample."""
    rng = np.random.default_rng(seed + 7)
    return (rng.normal(0, 1, ref.shape) / np.abs(ref).max()).astype(np.float32)
