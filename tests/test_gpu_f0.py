"""GPU parity of the f0 analysis (golf_f0_yin_f32, functional.f0_yin, f0.F0Analysis) against the float64 restatement of its
definition (tests/f0_ref.py, pinned on signals of known f0 by tests/test_f0_host.py) on the same fp32 inputs.

Bars: the project's parity bar, 1e-4, per frame with no frame left out -- period relative, f0 relative where the reference
is voiced and exactly 0 where it is not, ap absolute.  A frame whose integer lag or voicing differs from the reference is a
mismatch; a case may have them in 1 % of its frames, rounded down, so in none under 100 frames.  The fp32 stand-in of
tests/f0_ref.py has no such frame on these inputs (tests/test_f0_host.py)."""
import numpy as np
import pytest
import torch

import f0_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-4


def run(x, kw, strided=False, outputs="all"):
    """The case through functional.f0_yin, with the explicit lags of the case put as the frequencies that give them."""
    from golf_amd import functional as GF

    sr = kw["sample_rate"]
    f0_max, f0_min = sr / (kw["tau_min"] + 0.5), sr / (kw["tau_max"] - 0.5)
    assert GF.f0_lags(sr, f0_min, f0_max, kw["W"]) == (kw["tau_min"], kw["tau_max"], kw["W"])
    if strided:   # rows of a wider buffer: unit inner stride, row stride T + 37
        buf = torch.full((x.shape[0], x.shape[1] + 37), float("nan"), device="cuda")
        buf[:, : x.shape[1]] = torch.tensor(x)
        xd = buf[:, : x.shape[1]]
        assert not xd.is_contiguous()
    else:
        xd = x if isinstance(x, torch.Tensor) else torch.tensor(x).cuda()
    return GF.f0_yin(xd, sr, kw["hop"], f0_min, f0_max, kw["W"], kw.get("threshold", 0.15), kw.get("rms_floor", 0.0),
                     centred=kw.get("centred", True), n_frames=kw.get("F"), return_all=outputs == "all")


def compare(name, out, ref):
    f0, period, ap = (t.cpu().numpy().astype(np.float64) for t in out)
    assert f0.shape == period.shape == ap.shape == ref["f0"].shape
    assert np.isfinite(f0).all() and np.isfinite(period).all() and np.isfinite(ap).all()
    voiced = f0 > 0
    # The integer lag is not an output.  |delta| <= 1, so a period further than one sample from the reference's lag shows
    # another lag; every other frame is held to the bars below, also one whose lag differs unseen: stricter than the rule.
    flip = (np.abs(period - ref["tau"]) > 1.0) | (voiced != ref["voiced"])
    ok = ~flip
    e_p = (np.abs(period - ref["period"]) / ref["period"])[ok].max()
    e_ap = np.abs(ap - ref["ap"])[ok].max()
    both = ok & ref["voiced"]
    e_f0 = (np.abs(f0 - ref["f0"]) / np.where(ref["f0"] > 0, ref["f0"], 1.0))[both].max() if both.any() else 0.0
    print(f"{name}: {flip.size} frames, {int(flip.sum())} differ; period {e_p:.2e}  f0 {e_f0:.2e}  ap {e_ap:.2e}")
    assert int(flip.sum()) <= flip.size // 100
    assert (f0[ok & ~ref["voiced"]] == 0).all()
    assert e_p <= TOL and e_f0 <= TOL and e_ap <= TOL


@pytest.mark.parametrize("name", [n for n in R.cases()])
def test_parity_per_frame(name):
    x, kw = R.cases()[name]
    ref = R.reference(name)
    # the case is what it claims to be, in the reference, before anything is compared
    if name == "recipe":
        assert x.shape == (8, 4801) and ref["voiced"][:4, 4:-4].all() and not ref["voiced"][4].any()
    if name == "edges":
        assert x.shape[1] == 1000 < kw["W"] + kw["tau_max"]
    if name == "largest":
        assert kw["W"] + kw["tau_max"] == 16384 and kw["W"] % 8
    if name == "first_at_tau_min":
        assert (ref["first"] == kw["tau_min"]).any()
    if name == "star_at_tau_max":
        assert (ref["tau"] == kw["tau_max"]).any() and (ref["period"][ref["tau"] == kw["tau_max"]] == kw["tau_max"]).all()
    if name == "walk":
        assert ((ref["tau"] - ref["first"] > 1) & ref["found"]).any()
    if name == "fallback":
        assert not ref["found"].any()
    if name == "quiet_floor":
        assert R.reference("quiet")["voiced"].any() and not ref["voiced"].any()
    out = run(x, kw)
    assert all(t.dtype == torch.float32 and not t.requires_grad for t in out)
    compare(name, out, ref)
    if name == "more_frames":   # trailing frames of zeros: unvoiced, a finite period, ap = 1
        f0, period, ap = (t.cpu().numpy() for t in out)
        assert (f0[:, -4:] == 0).all() and (ap[:, -4:] == 1).all() and (period[:, -4:] == kw["tau_min"]).all()
    if name == "quiet_floor":   # the floor silences f0 and leaves period and ap as they were
        quiet = run(*R.cases()["quiet"])
        assert (out[0] == 0).all() and torch.equal(out[1], quiet[1]) and torch.equal(out[2], quiet[2])


def test_strided_rows():
    x, kw = R.cases()["small51"]
    out = run(x, kw, strided=True)
    compare("strided", out, R.reference("small51"))
    assert all(torch.equal(a, b) for a, b in zip(out, run(x, kw)))


def test_outputs_overwritten_and_null_outputs_untouched():
    """Through the C ABI: outputs pre-filled with NaN are written in full; a NULL period or ap is not written (the others
    come out the same), and the buffer next to an output keeps its NaNs."""
    from golf_amd import _lib

    lib = _lib.load()
    x, kw = R.cases()["small50"]
    ref = R.reference("small50")
    B, F = ref["f0"].shape
    xd = torch.tensor(x).cuda()
    S = kw["W"] + kw["tau_max"]

    def call(f0, period, ap):
        rc = lib.golf_f0_yin_f32(xd.data_ptr(), xd.stride(0), _lib.ptr(f0), _lib.ptr(period), _lib.ptr(ap), B, x.shape[1], F,
                                 kw["hop"], kw["W"], kw["tau_min"], kw["tau_max"], -(S // 2), kw["sample_rate"], 0.15, 0.0,
                                 _lib.stream_ptr())
        _lib.check(rc, "golf_f0_yin_f32")

    buf = torch.full((4, B, F), float("nan"), device="cuda")
    call(buf[0], buf[1], buf[2])
    assert torch.isfinite(buf[:3]).all() and torch.isnan(buf[3]).all()
    compare("abi", tuple(buf[:3]), ref)
    for keep in ((0,), (1,), (2,), (0, 2)):
        part = torch.full((4, B, F), float("nan"), device="cuda")
        call(*(part[i] if i in keep else None for i in range(3)))
        for i in range(4):
            assert torch.equal(part[i], buf[i]) if i in keep else torch.isnan(part[i]).all()


def test_bit_reproducible_and_batch_independent():
    x, kw = R.cases()["recipe"]
    xd = torch.tensor(x).cuda()
    first, second = run(xd, kw), run(xd, kw)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    for b in (0, 4, 7):
        alone = run(xd[b:b + 1], kw)
        assert all(torch.equal(a[0], t[b]) for a, t in zip(alone, first))
    swapped = run(xd.flip(0), kw)
    assert all(torch.equal(a.flip(0), t) for a, t in zip(swapped, first))


def test_graph_capture_replays_the_eager_result():
    x, kw = R.cases()["recipe"]
    xd = torch.tensor(x).cuda()
    eager = run(xd, kw)
    static = torch.zeros_like(xd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static, kw)                      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = run(static, kw)
    static.copy_(xd)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))


def test_autocast_grad_and_empty_batch():
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError

    x, kw = R.cases()["small50"]
    xd = torch.tensor(x).cuda()
    want = run(xd.bfloat16().float(), kw)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = run(xd.bfloat16(), kw)
    assert all(t.dtype == torch.float32 for t in got) and all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(GolfError, match="fp32"):
        run(xd.bfloat16(), kw)
    out = run(xd.clone().requires_grad_(True), kw)
    assert not any(t.requires_grad for t in out) and all(torch.equal(a, b) for a, b in zip(out, run(xd, kw)))
    f0 = run(xd.clone().requires_grad_(True), kw, outputs="f0")
    assert isinstance(f0, torch.Tensor) and not f0.requires_grad and torch.equal(f0, out[0])
    empty = GF.f0_yin(xd[:0], 8000.0, 7, 200.0, 2000.0, 50, return_all=True)
    assert len(empty) == 3 and all(t.shape == (0, 777 // 7 + 1) and t.is_cuda for t in empty)
    assert GF.f0_yin(xd[:0], 8000.0, 7, 200.0, 2000.0, 50, n_frames=9).shape == (0, 9)


def test_module():
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.f0 import F0Analysis

    x, kw = R.cases()["recipe"]
    ref = R.reference("recipe")
    xd = torch.tensor(x).cuda()
    m = F0Analysis(R.RECIPE["sr"], R.RECIPE["hop"], window_length=R.RECIPE["W"]).cuda()
    assert (m.tau_min, m.tau_max, m.window_length) == (kw["tau_min"], kw["tau_max"], kw["W"])
    f0 = m(xd)
    assert isinstance(f0, AudioTensor) and f0.hop_length == 240 and f0.shape == (8, 4801 // 240 + 1)
    three = m.analyse(AudioTensor(xd))
    compare("module", three, ref)
    assert torch.equal(three[0], f0.as_tensor())
    v = m.voicing(xd)
    assert isinstance(v, AudioTensor) and v.hop_length == 240 and v.as_tensor().dtype == torch.float32
    assert torch.equal(v.as_tensor(), (f0.as_tensor() > 0).float())
    assert torch.equal(v.as_tensor().cpu().bool(), torch.tensor(ref["voiced"]))
    with pytest.raises(AssertionError, match="hop 1"):
        m(AudioTensor(xd, 2))
