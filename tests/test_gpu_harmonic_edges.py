"""The harmonic oscillator bank (harm_kernel<DERIV>, harm_bwd_kernel, harm_bwd_combine_kernel behind functional.harmonic_osc)
on every operand subset, gradient, hop and tile edge of tests/harm_ref.py's case table, against that file's float64 closed
form.  Bars: 2e-5 for y and g_amp (what test_gpu_harmonic.py::test_vs_oracle holds against float64), 1e-4, the project's
parity bar, for g_phase, g_tscale, g_offset, g_initial_phase and dy/dPhi.  Every case's inputs keep h p at least 1e-6 away from
0.5 (or are planted exactly on it), so both sides evaluate the same Nyquist mask and no sample is left out of a comparison.
Every comparison prints the kernel's distances next to those of torch's own fp32 autograd through the dense formula on the
device: a case both miss is ill-conditioned and gets another input, never a wider bar."""
import numpy as np
import pytest
import torch

import harm_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

TRACKS = ("phase", "amp", "tscale", "offset", "initial_phase")
WORST = {}


def dev(x, grad=False):
    return None if x is None else torch.tensor(np.asarray(x), dtype=torch.float32).cuda().requires_grad_(grad)


def tensors(c, d=None, grads=None):
    """Device tensors of a case's inputs; the differentiable ones (all that exist, or ``grads``) are leaves."""
    d = R.inputs(c) if d is None else d
    want = [k[2:] for k in R.wanted(c) if k.startswith("g_")] if grads is None else grads
    t = {k: dev(d[k], k in want) for k in TRACKS}
    t["hscale"], t["gy"] = dev(d["hscale"]), dev(d["gy"])
    return t


def call(c, t):
    from golf_amd import functional as GF

    return GF.harmonic_osc(t["phase"], c.H, c.ph, t["amp"], c.ah, t["tscale"], c.sh, t["hscale"], t["offset"], c.oh,
                           t["initial_phase"])


def kernel(c, t, dphi=True, cotangent=None):
    """y, every gradient the leaves of ``t`` have, and dy/dPhi from golf_harmonic_osc_dphase_f32."""
    from golf_amd import _lib
    from golf_amd import functional as GF

    y = call(c, t)
    out = dict(y=y.detach())
    leaves = [k for k in TRACKS if t[k] is not None and t[k].requires_grad]
    if leaves:
        (y * t["gy"]).sum().backward() if cotangent is None else cotangent(y).backward()
        out.update({"g_" + k: t[k].grad for k in leaves})
    if dphi:
        geom = (c.H, c.ph, c.ah, c.sh, c.Fa or 1, c.Fs or 1, y.shape[1], bool(c.Fa))
        phase = t["phase"].detach()
        assert phase.is_contiguous()
        out["dphi"] = GF._HarmonicOsc._run(_lib.load(), "golf_harmonic_osc_dphase_f32", phase, t["amp"], t["tscale"],
                                           t["hscale"], geom, t["offset"], (c.Fo or 1, c.oh), t["initial_phase"])
    torch.cuda.synchronize()
    return out


def torch_fp32(c, t):
    """torch's own fp32 autograd through the dense formula on the device, on the same inputs."""
    u = {k: None if t[k] is None else t[k].detach().clone().requires_grad_(t[k].requires_grad) for k in TRACKS}
    eps = torch.zeros(c.B, t["gy"].shape[1], device="cuda", requires_grad=True)
    y = R.dense_torch(u["phase"], c.H, c.ph, u["amp"], c.ah, u["tscale"], c.sh, t["hscale"], u["offset"], c.oh,
                      u["initial_phase"], eps=eps)
    (dphi,) = torch.autograd.grad(y.sum(), eps, retain_graph=True)
    (y * t["gy"]).sum().backward()
    out = dict(y=y.detach(), dphi=dphi)
    out.update({"g_" + k: u[k].grad for k in TRACKS if u[k] is not None and u[k].requires_grad})
    return out


def compare(tag, got, ref, keys, bars=R.BARS, own=None, group=""):
    """Print every distance, then hold each to its bar."""
    missed = []
    for k in keys:
        g = got[k].detach().cpu().numpy()
        assert g.shape == ref[k].shape and np.isfinite(g).all(), (tag, k, g.shape, ref[k].shape)
        emax, el2 = rel_err(g, ref[k])
        line = f"{tag} {k}: kernel vs float64 rel-max {emax:.3e} L2 {el2:.3e} (bar {bars[k]:.0e})"
        if own is not None and k in own:
            o = rel_err(own[k].detach().cpu().numpy(), ref[k])
            line += f"; torch fp32 autograd on the device {o[0]:.3e} {o[1]:.3e}"
        print(line)
        WORST[group + k] = max(WORST.get(group + k, 0.0), emax, el2)
        if not (emax <= bars[k] and el2 <= bars[k]):
            missed.append((k, emax, el2))
    assert not missed, (tag, missed)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_case(c):
    """Forward, dy/dPhi and every gradient the case's operands have, against the float64 closed form."""
    g = R.geometry(c)
    ref = R.refs(c)
    t = tensors(c)
    keys = R.wanted(c)
    got = kernel(c, t, dphi="dphi" in keys)
    assert tuple(got["y"].shape) == (c.B, g.Tout)
    print(f"{c.name}: {c.edge}; seed +{R.inputs(c)['seed'] - c.seed} margin {R.margin(c):.2e} Tout {g.Tout} blocks {g.blocks} "
          f"tiles {g.tiles} segs {g.segs} lds {g.lds} ends {g.ends}")
    compare(c.name, got, ref, keys, own=torch_fp32(c, t))
    if c.Fa:   # rows no output sample touches: written, and exactly zero
        empty = R.empty_amp_rows(c)
        assert (ref["g_amp"][:, empty] == 0).all() and (got["g_amp"][:, empty] == 0).all(), empty


def test_hscale_gradient_is_refused():
    c = R.case("ops-a1s1h1o1i1")
    t = tensors(c)
    t["hscale"].requires_grad_(True)
    y = call(c, t)
    with pytest.raises(NotImplementedError):
        y.sum().backward()


@pytest.mark.parametrize("H,Fa,ah,ip,why", [
    (60, 300, 1, False, "rows"),       # amp_hop 1: 59 harmonics is the most the staged rows admit
    (3966, 0, 1, True, "lds"),         # one above the table's lds-max-noamp
    (2267, 3, 256, True, "lds"),       # one above the table's lds-max-amp256
    (3000, 3, 256, True, "lds"),       # 84 000 + 2 080 bytes: passed the row bound alone
    (4096, 0, 1, True, "lds"),         # 65 536 + 2 080 bytes
])
def test_refused_above_the_lds_limit(H, Fa, ah, ip, why):
    """A launch whose LDS request exceeds what the host admits is refused on the host (GOLF_EUNSUPPORTED = -3), forward and
    dy/dPhi alike; nothing is launched to find out."""
    from golf_amd import _lib
    from golf_amd import functional as GF

    assert R.refusal_of(H, Fa, ah, ip) == why and (R.lds_bytes_of(H, Fa, ah, ip) > R.LDS_LIMIT) == (why == "lds")
    T = R.up_len(Fa, ah) if Fa else 300
    phase = torch.full((1, T), 1e-4, device="cuda")
    amp = torch.ones(1, Fa, H, device="cuda") if Fa else None
    init = torch.zeros(1, H, device="cuda") if ip else None
    with pytest.raises(_lib.GolfError, match=r"bad argument -3: .*harmonics.*LDS staging"):
        GF.harmonic_osc(phase, H, 1, amp, ah, initial_phase=init)
    with pytest.raises(_lib.GolfError, match=r"bad argument -3: .*harmonics.*LDS staging"):
        GF._HarmonicOsc._run(_lib.load(), "golf_harmonic_osc_dphase_f32", phase, amp, None, None,
                             (H, 1, ah, 1, Fa or 1, 1, T, bool(Fa)), None, (1, 1), init)


def test_layouts():
    """A stride-0 cotangent (y.sum()), a phase and a tscale that are column slices of wider tensors and a non-contiguous
    amplitude tensor give the bits of the contiguous call."""
    c = R.case("ops-a1s1h1o1i1")
    d = R.inputs(c)
    base = kernel(c, tensors(c), dphi=False, cotangent=lambda y: (y * torch.ones_like(y)).sum())
    flat = kernel(c, tensors(c), dphi=False, cotangent=lambda y: y.sum())
    wide = {k: torch.randn(c.B, d[k].shape[1] + 7, device="cuda") for k in ("phase", "tscale")}
    holder = torch.randn(c.B, c.Fa, 2 * c.H, device="cuda")
    with torch.no_grad():
        for k in wide:
            wide[k][:, 3:3 + d[k].shape[1]] = dev(d[k])
        holder[:, :, ::2] = dev(d["amp"])
    t = tensors(c)
    for k in wide:
        wide[k].requires_grad_(True)
        t[k] = wide[k][:, 3:3 + d[k].shape[1]]
    holder.requires_grad_(True)
    t["amp"] = holder[:, :, ::2]
    assert not t["phase"].is_contiguous() and not t["tscale"].is_contiguous() and not t["amp"].is_contiguous()
    y = call(c, t)
    y.sum().backward()
    torch.cuda.synchronize()
    sliced = dict(y=y.detach(), g_phase=wide["phase"].grad[:, 3:3 + c.Tp], g_tscale=wide["tscale"].grad[:, 3:3 + c.Fs],
                  g_amp=holder.grad[:, :, ::2])
    for k in base:
        assert torch.equal(base[k], flat[k]), ("stride-0 cotangent", k)
    for k in sliced:
        assert torch.equal(base[k], sliced[k]), ("sliced operands", k)
    assert (holder.grad[:, :, 1::2] == 0).all() and (wide["phase"].grad[:, :3] == 0).all()


@pytest.mark.parametrize("name", ["ops-a1s1h1o1i1", "ops-a0s1h1o1i1", "H155", "unvoiced-ph16", "ph1-Tp2049"])
def test_deterministic(name):
    c = R.case(name)
    a, b = kernel(c, tensors(c)), kernel(c, tensors(c))
    assert set(a) == set(b) and len(a) >= 5
    for k in a:
        assert torch.equal(a[k], b[k]), (name, k)


@pytest.mark.parametrize("name", ["H65", "ops-a0s1h1o1i1"])
def test_rows_are_independent(name):
    """A voice's outputs and gradients have the same bits alone and as any row of a batch of three different voices."""
    c = R.case(name)._replace(B=3, name=name + "-three-voices")
    d = R.inputs(c)
    rowwise = [k for k in TRACKS + ("gy",) if d[k] is not None]

    def run(rows):
        sub = dict(d)
        sub.update({k: d[k][rows] for k in rowwise})
        return kernel(c._replace(B=len(rows)), tensors(c, sub))

    alone = [run([b]) for b in range(3)]
    for rows in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        batch = run(rows)
        for i, b in enumerate(rows):
            for k in batch:
                assert torch.equal(batch[k][i], alone[b][k][0]), (name, rows, b, k)


# ---- the modules ---------------------------------------------------------------------------------------------------------
def _module_reference(kind, c, d):
    """y, d/d phase, d/d amplitudes of a module in float64 CPU autograd through the dense formula."""
    f64 = lambda x, grad=False: torch.tensor(x, dtype=torch.float64).requires_grad_(grad)
    phase, amp = f64(d["phase"], True), f64(d["amp"], True)
    scale = torch.rsqrt(0.5 / phase)
    if kind == "additive":
        if c.ph == 1:      # synth.py:466-468: the product at the finer hop, here the sample rate
            y = R.dense_torch(phase, c.H, 1, amp, c.ah, tscale=scale, ts_hop=1)
        else:              # the amplitudes brought to the phase's hop, scaled there, then upsampled with the phase
            r = c.ah // c.ph
            fine = torch.nn.functional.interpolate(amp.transpose(1, 2), size=(c.Fa - 1) * r + 1, mode="linear",
                                                   align_corners=True).transpose(1, 2)
            n = min(fine.shape[1], c.Tp)
            y = R.dense_torch(phase, c.H, c.ph, fine[:, :n] * scale[:, :n, None], c.ph)
    elif kind == "saw":
        y = R.dense_torch(phase, c.H, c.ph, hscale=1 / torch.arange(1, c.H + 1, dtype=torch.float64))
    else:
        y = R.dense_torch(phase, c.H, c.ph, tscale=scale, ts_hop=c.ph)
    (y * f64(d["gy"][:, :y.shape[1]])).sum().backward()
    return dict(y=y.detach().numpy(), g_phase=phase.grad.numpy(), g_amp=None if amp.grad is None else amp.grad.numpy())


@pytest.mark.parametrize("kind", ["additive", "saw", "pulse"])
@pytest.mark.parametrize("name", [c.name for c in R.MODULE_CASES])
def test_modules(name, kind):
    """AdditiveSynthesizer (phase at hop 1: the scale rides as tscale; coarser: folded into the amplitudes), SawToothOscillator
    and AdditivePulseTrain: y, d/d phase and d/d amplitudes on mask-safe tracks."""
    from golf_amd.audiotensor import AudioTensor as AT
    from golf_amd import synth as S

    c = R.case(name)
    d = R.inputs(c)
    assert R.margin(c) >= R.MARGIN and (d["phase"] > 0).all()
    ref = _module_reference(kind, c, d)
    phase, amp = dev(d["phase"], True), dev(d["amp"], True)
    if kind == "additive":
        y = S.AdditiveSynthesizer(num_harmonics=c.H).cuda()(AT(phase, c.ph), AT(amp, c.ah)).as_tensor()
    elif kind == "saw":
        y = S.SawToothOscillator(num_harmonics=c.H).cuda()(AT(phase, c.ph)).as_tensor()
    else:
        y = S.AdditivePulseTrain(num_harmonics=c.H).cuda()(AT(phase, c.ph)).as_tensor()
    assert tuple(y.shape) == ref["y"].shape
    (y * dev(d["gy"][:, :y.shape[1]])).sum().backward()
    torch.cuda.synchronize()
    got = dict(y=y.detach(), g_phase=phase.grad, g_amp=amp.grad)
    keys = ["y", "g_phase"] + (["g_amp"] if kind == "additive" else [])
    assert (amp.grad is None) == (kind != "additive")
    compare(f"{kind} {name}", got, ref, keys, bars=dict(y=1e-4, g_phase=1e-4, g_amp=1e-4), group="modules ")


def test_worst_distances():
    """The worst distance per quantity over everything this file compared so far (the whole file: every table case)."""
    for k in sorted(WORST):
        print(f"worst {k}: {WORST[k]:.3e}")
    assert all(np.isfinite(v) for v in WORST.values())
