"""Device grouped reader (tzs_sorter_grouped / tzs_group_sorted).

The expected groups never come from the code under test.  For a sorter they
are the host path: tez_amd.ifile.read_stream over Sorter.output() of the same
sorter, grouped by the SAME_KEY-or-equal loop of the plugin's host reader,
and compared as five arrays, byte for byte and offset for offset.  For the
stand-alone call they are built in Python from the input records.
T = positions per tile of the flags pass and W = wide-compare key length (0
when there is none) come from group_geometry(), so the edge cases sit on the
kernels' real boundaries.
"""
import ctypes
import random
import zlib

import numpy as np
import pytest

from tez_amd import ifile

pytestmark = pytest.mark.gpu

BW = ifile.serialize_bytes_writable
TX = ifile.serialize_text
V = ifile.vint_write


@pytest.fixture(scope="module")
def engine():
    import __graft_entry__
    __graft_entry__.build()
    import tez_amd
    if not tez_amd.device_available():
        pytest.skip("no GPU")
    return tez_amd


@pytest.fixture(scope="module")
def geom(engine):
    return engine.group_geometry()


# ---- expectation ------------------------------------------------------------
def arrays_of(groups):
    """[(serialized key, [serialized values])] -> the five arrays."""
    key_off, val_off, group_off = [0], [0], [0]
    keys, vals = bytearray(), bytearray()
    for k, vs in groups:
        keys += k
        key_off.append(len(keys))
        for v in vs:
            vals += v
            val_off.append(len(vals))
        group_off.append(len(val_off) - 1)
    return (np.frombuffer(bytes(keys), dtype=np.uint8),
            np.array(key_off, dtype=np.uint64),
            np.frombuffer(bytes(vals), dtype=np.uint8),
            np.array(val_off, dtype=np.uint64),
            np.array(group_off, dtype=np.uint64))


def host_groups(recs):
    """The plugin's host loop over read_stream records, keys kept serialized."""
    groups = []
    prev = None
    for k, v, same in recs:
        if not same and (prev is None or k != prev):
            groups.append((k, []))
        groups[-1][1].append(v)
        prev = k
    return groups


def adjacent_groups(pairs):
    """Runs of adjacent equal keys of an in-memory record list."""
    return host_groups([(k, v, False) for k, v in pairs])


def stream_records(s, p):
    data, index = s.output()
    st, raw, cl = index[p]
    return ifile.read_stream(data[st:st + cl]) if cl else []


def check_arrays(got, groups, payload_bytes):
    """got = to_host() arrays; groups = expected [(key, [values])]."""
    key_data, key_off, val_data, val_off, group_off = got
    n = sum(len(vs) for _, vs in groups)
    assert group_off[0] == 0 and group_off[-1] == n
    assert np.all(np.diff(group_off.astype(np.int64)) > 0)
    assert np.all(np.diff(key_off.astype(np.int64)) >= 0)
    assert np.all(np.diff(val_off.astype(np.int64)) >= 0)
    assert key_off[0] == 0 and val_off[0] == 0
    assert key_off[-1] == len(key_data) and val_off[-1] == len(val_data)
    assert len(group_off) == len(key_off) == len(groups) + 1
    assert len(val_off) == n + 1
    per_group = np.diff(group_off.astype(np.int64)) * np.diff(key_off.astype(np.int64))
    assert int(per_group.sum()) + len(val_data) == payload_bytes
    want = arrays_of(groups)
    for name, g, w in zip(("key_data", "key_off", "val_data", "val_off", "group_off"),
                          got, want):
        assert g.dtype == w.dtype, name
        assert np.array_equal(g, w), name


def check_sorter(engine, s, P=1, counter=True):
    """Every partition of a flushed sorter against its own merged stream.
    Returns the expected groups per partition."""
    out = []
    total = 0
    for p in range(P):
        recs = stream_records(s, p)
        groups = host_groups(recs)
        payload = sum(len(k) + len(v) for k, v, _ in recs)
        total += payload
        g = s.grouped(p)
        try:
            assert g.n_records == len(recs)
            assert g.n_groups == len(groups)
            if not recs:
                assert not g.g.d_val_off and not g.g.d_key_data
                assert not g.g.d_group_off and not g.g.d_key_off and not g.g.d_val_data
            check_arrays(g.to_host(), groups, payload)
        finally:
            g.free()
            g.free()  # idempotent
        out.append(groups)
    if counter:
        assert s.counters()["output_bytes"] == total
    return out


def sorter_of(engine, spills, P=1, text=False, **conf):
    """spills: lists of (key, value[, partition]); all but the last are
    forced with spill(), flush() takes the last."""
    c = engine.make_conf(
        P, key_type=engine.KEY_TEXT if text else engine.KEY_BYTES,
        comparator=engine.CMP_TEXT if text else engine.CMP_TEZBYTES, **conf)
    s = engine.Sorter(c)
    for i, recs in enumerate(spills):
        for r in recs:
            s.write(r[0], r[1], r[2] if len(r) > 2 else -1)
        if i + 1 < len(spills):
            s.spill()
    s.flush()
    return s


def key4(i):
    return BW(int(i).to_bytes(4, "big"))


def val_of(i):
    return BW(b"v%d" % i)


# ---- counts -------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2])
@pytest.mark.parametrize("mode", ["equal", "unique"])
def test_counts(engine, n, mode):
    recs = [(key4(7 if mode == "equal" else i), val_of(i)) for i in range(n)]
    s = sorter_of(engine, [recs])
    groups = check_sorter(engine, s)[0]
    assert len(groups) == (min(n, 1) if mode == "equal" else n)
    s.close()


# ---- wave and tile boundaries ---------------------------------------------------
def _sizes(T):
    return sorted({63, 64, 65, T - 1, T, T + 1, 2 * T + 1})


def _boundary_keys(n, T):
    """Sorted keys whose group boundaries sit at 64k and T, and one either side."""
    cuts = set()
    for c in list(range(64, n, 64)) + [T]:
        cuts.update((c - 1, c, c + 1))
    gid, keys = 0, []
    for i in range(n):
        if i in cuts:
            gid += 1
        keys.append(gid)
    return keys


def test_sizes_across_wave_and_tile_boundaries(engine, geom):
    T, _ = geom
    for n in _sizes(T):
        ids = _boundary_keys(n, T)
        recs = [(key4(g), val_of(i)) for i, g in enumerate(ids)]
        random.Random(n).shuffle(recs)
        s = sorter_of(engine, [recs])
        groups = check_sorter(engine, s)[0]
        assert len(groups) == len(set(ids)), n
        s.close()
        # one group and n groups at the same sizes
        for mode in ("equal", "unique"):
            recs = [(key4(5 if mode == "equal" else i), val_of(i)) for i in range(n)]
            s = sorter_of(engine, [recs])
            groups = check_sorter(engine, s)[0]
            assert len(groups) == (1 if mode == "equal" else n), (n, mode)
            s.close()


# ---- long keys ------------------------------------------------------------------
def test_long_keys_differing_in_the_last_byte(engine, geom):
    _, W = geom
    recs = []
    i = 0
    for L in (9, 17, 25):  # agree in the first 8, 16, 24 content bytes
        for last in range(4):
            for _ in range(2):
                recs.append((TX(b"p" * (L - 1) + bytes([65 + last])), val_of(i)))
                i += 1
    s = sorter_of(engine, [recs], text=True)
    groups = check_sorter(engine, s)[0]
    assert len(groups) == 12 and all(len(vs) == 2 for _, vs in groups)
    s.close()
    for L in ([W - 1, W, W + 1] if W else []):  # runs of 40 equal keys around W
        assert L >= 5
        recs = []
        for run in range(3):  # serialized length L: 4-byte prefix + content
            k = BW(b"q" * (L - 5) + bytes([65 + run]))
            recs += [(k, val_of(len(recs) + j)) for j in range(40)]
        s = sorter_of(engine, [recs])
        groups = check_sorter(engine, s)[0]
        assert [len(vs) for _, vs in groups] == [40, 40, 40]
        s.close()


def test_one_run_of_1k_keys_then_a_last_byte_difference(engine):
    base = bytes(range(256)) * 4  # 1 KiB of content
    recs = [(BW(base), val_of(i)) for i in range(70)]
    recs.append((BW(base[:-1] + b"\x00"), val_of(70)))
    random.Random(3).shuffle(recs)
    s = sorter_of(engine, [recs])
    groups = check_sorter(engine, s)[0]
    assert sorted(len(vs) for _, vs in groups) == [1, 70]
    s.close()


# ---- key framing ----------------------------------------------------------------
@pytest.mark.parametrize("text", [True, False])
def test_prefix_keys_are_distinct_groups(engine, text):
    ser = TX if text else BW
    recs = []
    for i, c in enumerate((b"", b"a", b"ab", b"abc")):
        recs += [(ser(c), val_of(2 * i)), (ser(c), val_of(2 * i + 1))]
    random.Random(1).shuffle(recs)
    s = sorter_of(engine, [recs], text=text)
    groups = check_sorter(engine, s)[0]
    assert sorted(k for k, _ in groups) == sorted(ser(c) for c in (b"", b"a", b"ab", b"abc"))
    assert all(len(vs) == 2 for _, vs in groups)
    s.close()


# ---- values ---------------------------------------------------------------------
VLENS = (0, 1, 95, 96, 97, 4096)


def _value(i, ln):
    return bytes((i * 7 + j) & 0xFF for j in range(ln))


@pytest.mark.parametrize("shape", ["long", "short"])
def test_value_lengths_across_the_vector_store_threshold(engine, shape):
    """`long`: the average copy is long (a wave per record); `short`: many
    tiny records around the same long values (a half wave per record)."""
    recs = []
    for kc in (b"k", b"kk1", b"kkk22"):  # odd key lengths: odd value offsets
        for ln in VLENS + VLENS[::-1]:
            recs.append((TX(kc), _value(len(recs), ln)))
    if shape == "short":
        for i in range(2000):
            recs.append((TX(b"z%03d" % (i % 500)), _value(i, i % 3)))
    s = sorter_of(engine, [recs], text=True)
    groups = check_sorter(engine, s)[0]
    by_key = dict(groups)
    for kc in (b"k", b"kk1", b"kkk22"):
        assert sorted(len(v) for v in by_key[TX(kc)]) == sorted(VLENS + VLENS)
    s.close()


# ---- partitions and refusals ------------------------------------------------------
def test_three_partitions_with_an_empty_middle_one(engine):
    recs = [(key4(i % 9), val_of(i), 0 if i % 2 else 2) for i in range(300)]
    s = sorter_of(engine, [recs], P=3)
    groups = check_sorter(engine, s, P=3)
    assert len(groups[0]) > 0 and groups[1] == [] and len(groups[2]) > 0
    for bad in (3, -1):
        with pytest.raises(engine.EngineError, match="partition") as e:
            s.grouped(bad)
        assert e.value.rc == -22
    s.close()


def test_refused_before_flush_and_without_a_merged_set(engine):
    s = engine.Sorter(engine.make_conf(1))
    s.write(key4(1), val_of(1), -1)
    with pytest.raises(engine.EngineError, match="flush first") as e:
        s.grouped(0)
    assert e.value.rc == -22
    s.close()
    s = sorter_of(engine, [[(key4(1), val_of(1))], [(key4(2), val_of(2))]],
                  final_merge_enabled=0)
    assert s.num_spills() == 2
    with pytest.raises(engine.EngineError, match="final merge disabled") as e:
        s.grouped(0)
    assert e.value.rc == -22
    s.close()


# ---- several spills -------------------------------------------------------------
def _dup_spills(seed):
    rng = random.Random(seed)
    spills = []
    for sp in range(3):
        recs = []
        for j in range(400):
            kid = rng.randrange(60)  # duplicates inside and across spills
            recs.append((key4(kid), BW(b"s%d-%d" % (sp, j))))
        spills.append(recs)
    return spills


def test_three_spills_same_groups_whatever_the_rle_setting(engine):
    spills = _dup_spills(11)
    seen = []
    for rle in (0, 1, -1):
        s = sorter_of(engine, spills, rle=rle)
        assert s.num_spills() == 3
        seen.append(check_sorter(engine, s)[0])
        s.close()
    assert seen[0] == seen[1] == seen[2]
    assert len(seen[0]) == len({r[0] for sp in spills for r in sp})
    assert sum(len(vs) for _, vs in seen[0]) == 1200


def test_sum_combiner_leaves_one_value_per_group(engine):
    rng = random.Random(5)
    spills, want = [], {}
    for sp in range(3):
        recs = []
        for _ in range(500):
            k = TX(b"key%03d" % rng.randrange(40))
            v = rng.randrange(-50, 500)
            want[k] = want.get(k, 0) + v
            recs.append((k, v.to_bytes(4, "big", signed=True)))
        spills.append(recs)
    s = sorter_of(engine, spills, text=True, combiner=1, min_spills_for_combine=3)
    # OUTPUT_BYTES counts what was written, not the folded records
    groups = check_sorter(engine, s, counter=False)[0]
    assert all(len(vs) == 1 for _, vs in groups)
    assert {k: int.from_bytes(vs[0], "big", signed=True) for k, vs in groups} == want
    s.close()


@pytest.mark.parametrize("shape", ["c2_fixed", "c3_text"])
@pytest.mark.parametrize("nspill", [1, 2])
def test_generated_records_past_the_scan_threshold(engine, shape, nspill):
    """40 000 device-generated records: the offsets come from the single-pass
    scan (above 16 384 elements), and fixed-size records take the arithmetic
    record table, in one segment and in two."""
    n = 40000
    text = shape == "c3_text"
    conf = engine.make_conf(
        1, key_type=engine.KEY_TEXT if text else engine.KEY_BYTES,
        comparator=engine.CMP_TEXT if text else engine.CMP_TEZBYTES)
    s = engine.Sorter(conf)
    for k in range(nspill):
        d, off, kl, part = engine.generate(seed=0x6D + k, n=n // nspill,
                                           kind=1 if text else 0,
                                           klen=0 if text else 10, vlen=24, conf=conf)
        s.write_batch_device(d, off, kl, None, n // nspill)
        if k + 1 < nspill:
            s.spill()
        engine.free_device(d, off, kl, part)
    s.flush()
    groups = check_sorter(engine, s)[0]
    assert sum(len(vs) for _, vs in groups) == n
    if nspill == 1:
        assert len(groups) == n  # generated keys are unique within one set
    s.close()


# ---- IFile segment admission and the plugin ------------------------------------------
def _rec(k, v):
    return V(len(k)) + V(len(v)) + k + v


def _body(pairs, rle):
    out = bytearray()
    prev, in_run = None, False
    for k, v in pairs:
        if rle and prev is not None and k == prev:
            out += (b"" if in_run else b"\xfe") + V(len(v)) + v
            in_run = True
        else:
            if in_run:
                out += b"\xfd"
                in_run = False
            out += _rec(k, v)
        prev = k
    if in_run:
        out += b"\xfd"
    return bytes(out + b"\xff\xff")


def _frame(body):
    return b"TIF\x00" + body + zlib.crc32(body).to_bytes(4, "big")


def _four_segments():
    rng = random.Random(23)
    segs = []
    for i in range(4):
        pairs = sorted((key4(rng.randrange(50)), BW(b"m%d-%d" % (i, j)))
                       for j in range(200))
        segs.append(_frame(_body(pairs, rle=i % 2 == 1)))
    return segs


def test_ifile_segment_admission(engine):
    s = engine.Sorter(engine.make_conf(1))
    for seg in _four_segments():
        dev = engine.upload_bytes(seg)
        s.add_ifile_segment(dev, len(seg), partition=-1)
        engine.free_device(dev)
    s.flush()
    groups = check_sorter(engine, s)[0]
    assert sum(len(vs) for _, vs in groups) == 800
    s.close()


def test_plugin_reader_equals_the_host_reader(engine, monkeypatch):
    from tez_amd.ordered_input import GroupedKV, OrderedGroupedKVInput
    taken = []
    orig = OrderedGroupedKVInput._merge_resort
    monkeypatch.setattr(OrderedGroupedKVInput, "_merge_resort",
                        lambda self, payloads: taken.append(1) or orig(self, payloads))
    inp = OrderedGroupedKVInput(0)
    for seg in _four_segments():
        inp.add_segment(seg)
    inp.start()
    got = inp.get_reader()
    assert not taken
    assert got == inp.get_reader_host()
    assert isinstance(inp.get_grouped(), GroupedKV)
    assert len(inp.get_grouped()) == len(got) > 0
    assert sum(len(vs) for _, vs in got) == 800
    assert inp.get_grouped().key(0) == BW(got[0][0])
    assert inp.get_grouped().values(0) == got[0][1]
    inp.close()
    # variable-length BytesWritable keys in arrival order: not a sorted
    # segment, so the input decodes and re-sorts
    rng = random.Random(31)
    pairs = [(BW(bytes(rng.randrange(4) for _ in range(rng.randrange(0, 6)))),
              BW(b"r%d" % j)) for j in range(300)]
    inp = OrderedGroupedKVInput(0)
    inp.add_segment(_frame(_body(pairs[:150], rle=False)))
    inp.add_segment(_frame(_body(pairs[150:], rle=False)))
    inp.start()
    assert taken
    got = inp.get_reader()
    assert got == inp.get_reader_host()
    assert sorted(k for k, _ in got) == sorted({k[4:] for k, _ in pairs})
    assert sum(len(vs) for _, vs in got) == 300
    inp.close()
    # nothing fetched: no groups
    inp = OrderedGroupedKVInput(0).start()
    assert inp.get_reader() == [] and inp.get_reader_host() == []
    inp.close()


# ---- the stand-alone call --------------------------------------------------------
def _group_sorted(engine, pairs, text=False, shift=0):
    data = b"".join(k + v for k, v in pairs)
    off = np.cumsum([0] + [len(k) + len(v) for k, v in pairs]).astype(np.uint64)
    klen = np.array([len(k) for k, _ in pairs], dtype=np.uint32)
    d, o_, kl, _ = engine.upload_records(b"\xa5" * shift + data, off, klen)
    conf = engine.make_conf(
        1, key_type=engine.KEY_TEXT if text else engine.KEY_BYTES,
        comparator=engine.CMP_TEXT if text else engine.CMP_TEZBYTES)
    try:
        g = engine.group_sorted(conf, (ctypes.c_void_p(d.value + shift), o_, kl,
                                       len(pairs)))
        try:
            assert g.n_records == len(pairs)
            return g.to_host()
        finally:
            g.free()
    finally:
        engine.free_device(d, o_, kl)


@pytest.mark.parametrize("shift", [0, 1, 2, 3, 7])
def test_group_sorted_on_a_sorted_segment(engine, geom, shift):
    T, _ = geom
    pairs = []
    for g in range(40):
        k = TX(b"w%02d" % g + b"x" * (g % 5))
        for j in range(1 + (g * 7) % 23):
            pairs.append((k, _value(len(pairs), VLENS[(g + j) % len(VLENS)])))
    assert len(pairs) > T
    groups = adjacent_groups(pairs)
    assert len(groups) == 40
    check_arrays(_group_sorted(engine, pairs, text=True, shift=shift), groups,
                 sum(len(k) + len(v) for k, v in pairs))


def test_group_sorted_groups_adjacent_runs_only(engine):
    a, b = key4(1), key4(2)
    pairs = [(a, val_of(0)), (a, val_of(1)), (b, val_of(2)), (a, val_of(3))]
    groups = adjacent_groups(pairs)
    assert [k for k, _ in groups] == [a, b, a]  # the recurrence is a new group
    check_arrays(_group_sorted(engine, pairs), groups,
                 sum(len(k) + len(v) for k, v in pairs))
    g = engine.group_sorted(engine.make_conf(1), (None, None, None, 0))
    assert g.n_records == 0 and g.n_groups == 0 and not g.g.d_val_off
    g.free()
