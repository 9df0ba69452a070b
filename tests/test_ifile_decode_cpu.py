"""CPU-runnable checks of the device IFile decoder's host side: geometry,
argument validation ahead of any device call, and the plugin input no longer
pushing fetched records through the per-record host write path."""
import ctypes
import inspect
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(REPO, "tez_amd", "libtezsort.so")


def _lib():
    if not os.path.exists(SO):
        import __graft_entry__
        __graft_entry__.build()
    from tez_amd._engine import lib
    return lib()


def test_geometry_is_published():
    from tez_amd import _engine
    _lib()
    chunk, group = _engine.ifile_decode_geometry()
    assert chunk >= 64 and chunk & (chunk - 1) == 0, chunk
    assert group >= 2, group


def _decode_rc(L, ptr, nbytes, flags):
    d, o, k = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    n = ctypes.c_int64(-7)
    rc = L.tzs_ifile_decode(ptr, nbytes, flags, ctypes.byref(d), ctypes.byref(o),
                            ctypes.byref(k), ctypes.byref(n))
    return rc, L.tzs_last_error().decode()


def test_argument_validation_needs_no_device():
    L = _lib()
    # a host address: never dereferenced, validation comes first
    buf = ctypes.create_string_buffer(16)
    ptr = ctypes.addressof(buf)
    rc, msg = _decode_rc(L, ptr, -1, 1)
    assert rc == -22 and "nbytes" in msg
    rc, msg = _decode_rc(L, ptr, 16, 2)  # verify without header/trailer
    assert rc == -22 and "CRC" in msg
    rc, msg = _decode_rc(L, ptr, 16, 8)
    assert rc == -22 and "flags" in msg
    rc, msg = _decode_rc(L, ptr, 1 << 31, 1)
    assert rc == -22 and "too large" in msg
    rc, msg = _decode_rc(L, ptr, 7, 3)  # no room for header + trailer
    assert rc == -22 and "truncated" in msg
    rc, msg = _decode_rc(L, None, 16, 1)
    assert rc == -22 and "null" in msg


def test_add_ifile_segment_validates_before_touching_the_sorter():
    L = _lib()
    buf = ctypes.create_string_buffer(16)
    assert L.tzs_sorter_add_ifile_segment(None, ctypes.addressof(buf), 16, 1, -1) == -22
    assert "null sorter" in L.tzs_last_error().decode()


def test_plugin_input_has_no_per_record_write_loop():
    from tez_amd.ordered_input import OrderedGroupedKVInput
    cls_src = inspect.getsource(OrderedGroupedKVInput)
    start_src = inspect.getsource(OrderedGroupedKVInput.start)
    assert ".write(" not in start_src
    assert ".write(" not in cls_src
    # fetched inputs are parsed on the device, not by the Python reader
    assert "add_ifile_segment" in cls_src
    assert cls_src.count("read_stream") == 1  # the merged output only
