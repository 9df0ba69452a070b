"""CPU-runnable checks of the grouped reader's host side: the GroupedKV
container over hand-written arrays, argument validation of the C entry points
ahead of any device call, the published geometry, and the plugin input no
longer parsing the merged stream in start()."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from tez_amd import ifile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(REPO, "tez_amd", "libtezsort.so")


def _lib():
    if not os.path.exists(SO):
        import __graft_entry__
        __graft_entry__.build()
    from tez_amd._engine import lib
    return lib()


def _arrays(groups):
    """groups: [(serialized key, [serialized values])] -> the five arrays."""
    key_off, val_off, group_off = [0], [0], [0]
    keys, vals = b"", b""
    for k, vs in groups:
        keys += k
        key_off.append(len(keys))
        for v in vs:
            vals += v
            val_off.append(len(vals))
        group_off.append(len(val_off) - 1)
    return (np.frombuffer(keys, dtype=np.uint8), np.array(key_off, dtype=np.uint64),
            np.frombuffer(vals, dtype=np.uint8), np.array(val_off, dtype=np.uint64),
            np.array(group_off, dtype=np.uint64))


BW = ifile.serialize_bytes_writable
TX = ifile.serialize_text


def test_groupedkv_bytes_keys():
    from tez_amd.ordered_input import GroupedKV
    groups = [(BW(b""), [BW(b"x"), b"", BW(b"yy")]),     # empty-content key, empty value
              (BW(b"a"), [b""]),
              (BW(b"ab"), [BW(b"1"), BW(b"2")]),
              (BW(b"b" * 300), [b"", b"", BW(b"z" * 200)])]
    g = GroupedKV(*_arrays(groups))
    assert len(g) == 4
    assert list(g) == [(k[4:], vs) for k, vs in groups]
    for i, (k, vs) in enumerate(groups):
        assert g.key(i) == k
        assert g.values(i) == vs
    with pytest.raises(IndexError):
        g.key(4)


def test_groupedkv_text_keys():
    from tez_amd.ordered_input import GroupedKV
    long_key = b"k" * 200  # two-byte vint prefix
    groups = [(TX(b""), [b"\0\0\0\1"]),
              (TX(b"a"), [b"\0\0\0\1", b"\0\0\0\2"]),
              (TX(b"ab"), [b""]),
              (TX(long_key), [b"\0\0\0\3"])]
    g = GroupedKV(*_arrays(groups), text_keys=True)
    assert len(g) == 4
    assert list(g) == [(b"", [b"\0\0\0\1"]), (b"a", [b"\0\0\0\1", b"\0\0\0\2"]),
                       (b"ab", [b""]), (long_key, [b"\0\0\0\3"])]
    assert g.key(3) == TX(long_key)


def test_groupedkv_one_record_per_group():
    from tez_amd.ordered_input import GroupedKV
    groups = [(BW(bytes([i])), [BW(bytes([i, i]))]) for i in range(5)]
    g = GroupedKV(*_arrays(groups))
    assert list(g) == [(bytes([i]), [BW(bytes([i, i]))]) for i in range(5)]


def test_groupedkv_single_group_and_zero_groups():
    from tez_amd.ordered_input import GroupedKV
    one = [(TX(b"only"), [b"1", b"", b"333"])]
    g = GroupedKV(*_arrays(one), text_keys=True)
    assert len(g) == 1 and list(g) == [(b"only", [b"1", b"", b"333"])]
    z = np.zeros(1, dtype=np.uint64)
    e = np.zeros(0, dtype=np.uint8)
    g0 = GroupedKV(e, z, e, z, z)
    assert len(g0) == 0 and list(g0) == []
    with pytest.raises(IndexError):
        g0.key(0)


def test_argument_validation_needs_no_device():
    from tez_amd._engine import TzsConf, TzsGroups, TzsSegment
    L = _lib()
    out = TzsGroups()
    assert L.tzs_sorter_grouped(None, 0, ctypes.byref(out)) == -22
    assert "null sorter" in L.tzs_last_error().decode()
    # a host address standing in for a sorter: never dereferenced, the null
    # output is refused first
    fake = ctypes.create_string_buffer(64)
    assert L.tzs_sorter_grouped(ctypes.addressof(fake), 0, None) == -22
    assert "null output" in L.tzs_last_error().decode()

    conf = TzsConf()
    L.tzs_conf_default(ctypes.byref(conf), 1)
    seg = TzsSegment()
    seg.n = -1
    assert L.tzs_group_sorted(ctypes.byref(conf), ctypes.byref(seg),
                              ctypes.byref(out)) == -22
    assert "negative n" in L.tzs_last_error().decode()
    seg.n = 3  # columns left null
    assert L.tzs_group_sorted(ctypes.byref(conf), ctypes.byref(seg),
                              ctypes.byref(out)) == -22
    assert "null columns" in L.tzs_last_error().decode()
    buf = ctypes.create_string_buffer(64)
    seg.d_data = ctypes.addressof(buf)
    seg.d_off = ctypes.addressof(buf)  # d_klen still null
    assert L.tzs_group_sorted(ctypes.byref(conf), ctypes.byref(seg),
                              ctypes.byref(out)) == -22
    assert "null columns" in L.tzs_last_error().decode()
    assert L.tzs_group_sorted(ctypes.byref(conf), ctypes.byref(seg), None) == -22
    assert "null output" in L.tzs_last_error().decode()
    assert L.tzs_group_sorted(None, ctypes.byref(seg), ctypes.byref(out)) == -22
    assert L.tzs_group_sorted(ctypes.byref(conf), None, ctypes.byref(out)) == -22


def test_groups_free_of_zeroed_struct_is_harmless():
    from tez_amd._engine import Groups, TzsGroups
    L = _lib()
    g = TzsGroups()
    L.tzs_groups_free(ctypes.byref(g))
    L.tzs_groups_free(ctypes.byref(g))
    L.tzs_groups_free(None)
    assert g.n_records == 0 and not g.d_val_off and not g.d_key_data
    h = Groups(TzsGroups())
    h.free()
    h.free()
    kd, ko, vd, vo, go = h.to_host()
    assert len(kd) == 0 and len(vd) == 0
    assert ko.tolist() == [0] and vo.tolist() == [0] and go.tolist() == [0]


def test_geometry_is_published():
    from tez_amd import _engine
    _lib()
    tile, wide = _engine.group_geometry()
    assert tile > 0
    assert wide >= 0


def test_start_does_not_parse_the_merged_stream():
    from tez_amd.ordered_input import OrderedGroupedKVInput
    assert "read_stream" not in inspect.getsource(OrderedGroupedKVInput.start)
    assert "grouped(" in inspect.getsource(OrderedGroupedKVInput.start)
    host_src = inspect.getsource(OrderedGroupedKVInput.get_reader_host)
    assert host_src.count("read_stream") == 1
