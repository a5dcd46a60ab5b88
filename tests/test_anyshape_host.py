"""Host side of the sample-wise filter's shapes off the ring grid (csrc/lpc_any.hip): no GPU needed."""


def test_every_shape_has_a_backward():
    from golf_amd.functional import ss_has_backward

    assert ss_has_backward(22, 100) and ss_has_backward(64, 7) and ss_has_backward(31, 256)
    assert ss_has_backward(22, 240, F=1)
    assert not ss_has_backward(65, 240) and not ss_has_backward(0, 240)


def test_ring_grid_is_unchanged():
    from golf_amd.functional import ss_is_trainable

    assert ss_is_trainable(22, 240) and ss_is_trainable(26, 240) and ss_is_trainable(38, 240) and ss_is_trainable(30, 256)
    assert not ss_is_trainable(39, 240) and not ss_is_trainable(22, 100) and not ss_is_trainable(31, 256)
    assert not ss_is_trainable(22, 240, F=1)


def test_offgrid_workspace_size():
    from golf_amd import _lib

    lib = _lib.load()
    assert lib.golf_ltv_allpole_workspace_bytes_ex(0, 1, 1, 1, 1, 0) == 0
    n = lib.golf_ltv_allpole_workspace_bytes_ex(2, 801, 9, 22, 100, 0)
    assert n >= 256 and n % 256 == 0
    assert n >= 2 * 801 * 4   # the adjoint's g (B, T) lives there between the two backward kernels


def test_offgrid_backward_checks_its_arguments():
    """Rejected before any launch, so safe without a GPU: null pointers first, M > 64 unsupported, then the workspace."""
    from golf_amd import _lib

    lib = _lib.load()
    rc = lib.golf_ltv_allpole_bwd_f32(None, 0, None, 0, None, 0, None, None, None, 0, None, None, 2, 801, 9, 22, 100, None, 0, 0,
                                      None)
    assert rc == -1 and b"null pointer" in lib.golf_last_error()
    rc = lib.golf_ltv_allpole_bwd_f32(None, 0, None, 0, None, 0, None, None, None, 0, None, None, 2, 801, 9, 65, 100, None, 0, 0,
                                      None)
    assert rc == -3
    one = 1 << 12   # any non-null address: the workspace check comes before the first dereference
    rc = lib.golf_ltv_allpole_bwd_f32(one, 801, one, 801, one, 801, one, one, one, 801, one, one, 2, 801, 9, 22, 100, None, 0, 0,
                                      None)
    assert rc == -2 and b"workspace" in lib.golf_last_error()


def test_translation_unit_is_built():
    from golf_amd import _lib

    assert "lpc_any.hip" in _lib.SOURCES
