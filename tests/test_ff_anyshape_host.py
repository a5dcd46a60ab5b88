"""CPU: the frame-wise filter off the ring grid (csrc/lpc_ff_any.hip) -- what can be checked without a launch: the source
list, the host predicate that restates the routing rule, the order of the two C entries' argument checks at orders past the
ring grid, and the backward's workspace size."""
import ctypes


def test_source_list():
    from golf_amd import _lib

    assert "lpc_ff_any.hip" in _lib.SOURCES


def test_ring_grid_predicate():
    from golf_amd.functional import ff_on_ring_grid

    # the unchanged grid
    assert ff_on_ring_grid(22, 240, 960) and ff_on_ring_grid(26, 120, 480) and ff_on_ring_grid(38, 240, 960)
    assert ff_on_ring_grid(22, 240, 960, backward=True) and ff_on_ring_grid(26, 120, 480, backward=True)
    assert ff_on_ring_grid(38, 240, 960, backward=True)
    # off it: order past 38, hop below the ring width of the order
    assert not ff_on_ring_grid(39, 240) and not ff_on_ring_grid(22, 16) and not ff_on_ring_grid(30, 30)
    assert not ff_on_ring_grid(64, 240, 960, backward=True) and not ff_on_ring_grid(5, 4, 8)
    # a window that is no multiple of the ring width: ring forward, wave-per-frame backward
    assert not ff_on_ring_grid(22, 240, 1000, backward=True)
    assert ff_on_ring_grid(22, 240, 1000) and ff_on_ring_grid(22, 240, 1000, backward=False)
    # the ring chain's g_a kernel stages two whole frames per wave: 16*(2*W + ring + 6) bytes have to fit 64 KB
    assert ff_on_ring_grid(22, 240, 2016, backward=True) and not ff_on_ring_grid(22, 240, 2040, backward=True)


def _entries():
    from golf_amd import _lib

    lib = _lib.load()
    one = ctypes.c_void_p(256)   # never dereferenced: every call below is refused on its arguments
    B, F, hop, W = 2, 7, 240, 960
    Tx = (F - 1) * hop + 1
    Ty = (F - 1) * hop

    def fwd(M, p, ws_bytes):
        return lib.golf_lti_frames_ola_fwd_f32(p, Tx, p, p, p, p, Ty, B, Tx, F, M, hop, W, Ty, p, ws_bytes, None)

    def bwd(M, p, ws_bytes):
        return lib.golf_lti_frames_ola_bwd_f32(p, Ty, p, Tx, p, p, p, p, Tx, Tx, p, p, B, Tx, F, M, hop, W, Ty, p, p, ws_bytes,
                                               None)

    return lib, one, (("fwd", fwd), ("bwd", bwd))


def test_entries_check_arguments_before_the_order():
    lib, one, entries = _entries()
    for name, f in entries:
        assert f(64, None, 1 << 40) == -1, name
        assert b"null pointer" in lib.golf_last_error(), (name, lib.golf_last_error())
        assert f(64, one, 256) == -2, name
        assert b"workspace" in lib.golf_last_error(), (name, lib.golf_last_error())
        assert f(65, one, 1 << 40) == -3, name
        assert b"64" in lib.golf_last_error(), (name, lib.golf_last_error())
        # the order limit does not overtake the argument checks
        assert f(65, None, 1 << 40) == -1 and f(65, one, 256) == -2, name


def test_backward_workspace_size():
    from golf_amd import _lib

    lib = _lib.load()
    n = lib.golf_lti_frames_bwd_workspace_bytes(2, 1441, 7, 64, 240, 1000)
    assert n > 0 and n % 256 == 0
    # g_q (B, Ty), u_f (B, nfr, W) and the gain partial sums, each rounded up to 256 bytes: no more off the grid than on it
    assert n == lib.golf_lti_frames_bwd_workspace_bytes(2, 1441, 7, 22, 240, 1000)
    assert lib.golf_lti_frames_workspace_bytes(2, 1441, 7, 64, 240, 1000) == -(-4 * 2 * 7 * 1000 // 256) * 256
