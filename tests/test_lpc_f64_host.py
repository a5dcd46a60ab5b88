"""CPU: the float64 sample-wise filter's C entries (golf_ltv_allpole_{fwd,bwd}_f64, csrc/lpc_any.hip) refuse bad arguments
before any launch, and its Python entrances check dtypes and devices before they touch a device."""
import pytest
import torch


def lib():
    from golf_amd import _lib

    _lib.build()
    return _lib.load()


def test_workspace_bytes():
    L = lib()
    assert L.golf_ltv_allpole_f64_workspace_bytes(32, 47761) >= 32 * 47761 * 8
    assert L.golf_ltv_allpole_f64_workspace_bytes(32, 47761) % 256 == 0
    assert L.golf_ltv_allpole_f64_workspace_bytes(0, 47761) == 0
    assert L.golf_ltv_allpole_f64_workspace_bytes(1, 1) == 256


def fwd(L, B=2, T=10, F=3, M=4, hop=8, io=1, ptr=None):
    return L.golf_ltv_allpole_fwd_f64(ptr, T, ptr, ptr, ptr, T, B, T, F, M, hop, None, io, None)


def bwd(L, B=2, T=10, F=3, M=4, hop=8, io=1, ptr=None, ws=None, ws_bytes=0):
    return L.golf_ltv_allpole_bwd_f64(ptr, T, ptr, T, ptr, T, ptr, ptr, None, ptr, T, T, ptr, ptr, None, B, T, F, M, hop, ws,
                                      ws_bytes, io, None)


@pytest.mark.parametrize("call", [fwd, bwd])
def test_refusals_before_any_launch(call):
    """Null pointers throughout: every refusal below comes back before a kernel could be launched."""
    L = lib()
    assert call(L) == -1 and b"null" in L.golf_last_error()
    for bad in (dict(B=0), dict(T=0), dict(F=0), dict(M=0), dict(hop=0), dict(B=-3)):
        assert call(L, **bad) == -1 and b"non-positive" in L.golf_last_error(), bad
    assert call(L, T=100, hop=10) == -1 and b"exceeds" in L.golf_last_error()     # (F-1)*hop+1 = 21
    assert call(L, T=17, hop=8) == -1 and b"null" in L.golf_last_error()         # the last admissible length
    for io in (2, -1):
        assert call(L, io=io) == -1 and b"io=" in L.golf_last_error()
    assert call(L, io=0) == -1 and b"null" in L.golf_last_error()
    assert call(L, M=65, hop=80) == -3 and b"64" in L.golf_last_error()
    assert call(L, M=64, hop=80) == -1 and b"null" in L.golf_last_error()


def test_backward_refuses_a_small_workspace_and_narrow_rows():
    """With non-null (never dereferenced: the refusal comes first) pointers the backward gets as far as its workspace."""
    L = lib()
    fake = 1 << 20   # 256-aligned, host side only
    need = L.golf_ltv_allpole_f64_workspace_bytes(2, 10)
    assert bwd(L, ptr=fake, ws=None, ws_bytes=need) == -1 and b"workspace" in L.golf_last_error()
    assert bwd(L, ptr=fake, ws=fake, ws_bytes=need - 1) == -1 and b"workspace" in L.golf_last_error()
    assert bwd(L, ptr=fake, ws=fake + 8, ws_bytes=need) == -1 and b"workspace" in L.golf_last_error()
    rc = L.golf_ltv_allpole_bwd_f64(fake, 9, fake, 10, fake, 10, fake, fake, None, fake, 10, 10, fake, fake, None, 2, 10, 3, 4, 8,
                                    fake, need, 1, None)
    assert rc == -1 and b"stride" in L.golf_last_error()
    rc = L.golf_ltv_allpole_bwd_f64(fake, 10, fake, 10, fake, 10, fake, fake, None, fake, 11, 12, fake, fake, None, 2, 10, 3, 4,
                                    8, fake, need, 1, None)
    assert rc == -1 and b"width" in L.golf_last_error()
    rc = L.golf_ltv_allpole_fwd_f64(fake, 10, fake, fake, fake, 9, 2, 10, 3, 4, 8, None, 0, None)
    assert rc == -1 and b"stride" in L.golf_last_error()


def test_mixed_dtypes_raise_before_the_device_check():
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError

    ex, gain, a, zi = torch.zeros(1, 50), torch.ones(1, 3), torch.zeros(1, 3, 4), torch.zeros(1, 4)
    for k in range(4):
        ts = [t.double() if i == k else t for i, t in enumerate((ex, gain, a, zi))]
        with pytest.raises(GolfError, match="dtype") as e:
            GF.ltv_allpole_ss(ts[0], ts[1], ts[2], 24, zi=ts[3])
        assert "torch.float64" in str(e.value) and "torch.float32" in str(e.value) and "zi is" in str(e.value)
        with pytest.raises(GolfError, match="dtype"):
            GF.ltv_allpole_ss_blocks(ts[0], ts[1], ts[2], 24, 1, zi=ts[3])
    with pytest.raises(GolfError, match="dtype"):
        GF.ltv_allpole_ss(ex.double(), gain, a.double(), 24, mode="fp64")


def test_double_cpu_tensors_have_no_cpu_path():
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError

    ex, gain, a = torch.zeros(1, 50).double(), torch.ones(1, 3).double(), torch.zeros(1, 3, 4).double()
    with pytest.raises(GolfError, match="no CPU path"):
        GF.ltv_allpole_ss(ex, gain, a, 24)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.ltv_allpole_ss(ex, gain, a, 24, zi=torch.zeros(1, 4).double(), return_zf=True)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.ltv_allpole_ss(ex.float(), gain.float(), a.float(), 24, mode="fp64")
    with pytest.raises(GolfError, match="no CPU path"):
        GF.ltv_allpole_ss_blocks(ex, gain, a, 24, 1)
    with pytest.raises(GolfError, match="no CPU path"):   # the empty batch takes doubles too, and checks the device all the same
        GF.ltv_allpole_ss(ex[:0], gain[:0], a[:0], 24)


def test_status_belongs_to_the_chunked_scan():
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError

    ex, gain, a = torch.zeros(1, 50), torch.ones(1, 3), torch.zeros(1, 3, 4)
    st = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(GolfError, match="chunked"):
        GF.ltv_allpole_ss(ex.double(), gain.double(), a.double(), 24, status=st)
    with pytest.raises(GolfError, match="chunked"):
        GF.ltv_allpole_ss(ex, gain, a, 24, mode="fp64", status=st)


def test_require_device_admits_float64_only_when_asked():
    from golf_amd import _lib

    with pytest.raises(_lib.GolfError, match="no CPU path"):
        _lib.require_device(torch.zeros(2).double(), dtype=torch.float64)
    if torch.cuda.is_available():
        d = torch.zeros(2, device="cuda").double()
        _lib.require_device(d, dtype=torch.float64)
        with pytest.raises(_lib.GolfError, match="fp32"):
            _lib.require_device(d)


def test_module_precision_attribute():
    from golf_amd import functional as GF
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import LTVMinimumPhaseFilterPrecise

    assert GF.ss_has_f64(22, 240, 200) and GF.ss_has_f64(64, 7, 1) and not GF.ss_has_f64(65, 240, 200)
    filt = LTVMinimumPhaseFilterPrecise(lpc_order=4)
    assert filt.precision == "fp32" and LTVMinimumPhaseFilterPrecise.precision == "fp32"
    args = (AudioTensor(torch.zeros(1, 50)), AudioTensor(torch.ones(1, 3), 24), AudioTensor(torch.zeros(1, 3, 4), 24))
    filt.precision = "double"
    with pytest.raises(ValueError, match="precision"):
        filt(*args)
    filt.precision = "fp64"
    with pytest.raises(GF._lib.GolfError, match="no CPU path"):   # a valid value gets as far as the device check
        filt(*args)
    assert LTVMinimumPhaseFilterPrecise(lpc_order=4).precision == "fp32"   # per instance
