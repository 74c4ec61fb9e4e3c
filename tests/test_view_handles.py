"""CPU: a view handle is looked up among the live views before anything is read through it (include/imt.h), so a handle
that is not a view -- here a buffer of ones, standing for a freed view or another kind of handle -- is an argument error
to every imt_itree_view_* call.  No GPU is involved: the refusal comes before the first device call."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -9


def test_foreign_view_handle_is_refused():
    lib = ctypes.CDLL(os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc", "libimt_hip.so"))
    vp, sz, u = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint
    lib.imt_itree_view_size.restype = ctypes.c_uint64
    lib.imt_itree_view_free.restype = None
    junk = ctypes.create_string_buffer(b"\x01" * 4096, 4096)
    buf, idx, st = ctypes.create_string_buffer(4096), (ctypes.c_uint64 * 8)(), (ctypes.c_uint8 * 8)()
    for bad in (ctypes.cast(junk, vp), vp(None)):
        for flags in (0, 3, 0x10):
            assert lib.imt_itree_view_root(bad, buf, u(flags)) == ERR_ARG
            assert lib.imt_itree_view_lookup_batch(bad, buf, sz(1), st, idx, u(flags)) == ERR_ARG
            assert lib.imt_itree_view_get_leaves(bad, idx, sz(1), buf, u(flags)) == ERR_ARG
            assert lib.imt_itree_view_get_proof_batch(bad, idx, sz(1), buf, u(flags)) == ERR_ARG
            assert lib.imt_itree_view_non_membership_witness(bad, buf, sz(1), idx, buf, st, buf, u(flags)) == ERR_ARG
        assert lib.imt_itree_view_stats(bad, idx, idx) == ERR_ARG
        assert lib.imt_itree_view_size(bad) == 0
        lib.imt_itree_view_free(bad)
    assert junk.raw == b"\x01" * 4096
