"""Device IFile reader (tzs_ifile_decode / tzs_sorter_add_ifile_segment).

Every decode is compared byte for byte (d_data, d_off, d_klen, n) with the
columnar arrays rebuilt from oracle.ifile_read, which is itself cross-checked
against tez_amd.ifile.read_stream on the same bytes.  C = chunk bytes and
G = chunks per group come from ifile_decode_geometry(), so the edge cases sit
on the decoder's real chunk and group boundaries.
"""
import collections
import ctypes
import os
import random
import zlib

import numpy as np
import pytest

import oracle as o
from tez_amd import ifile

pytestmark = pytest.mark.gpu

V = ifile.vint_write
EOF = b"\xff\xff"
RLE = b"\xfe"
V_END = b"\xfd"


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
    return engine.ifile_decode_geometry()


# ---- stream builders ------------------------------------------------------
def rec(k, v):
    return V(len(k)) + V(len(v)) + k + v


def frame(body):
    return b"TIF\x00" + body + zlib.crc32(body).to_bytes(4, "big")


def write_body(pairs, rle=True):
    """IFile.Writer framing (IFile.java:590-615): equal consecutive keys go
    out as RLE_MARKER + continuations, closed by V_END."""
    out = bytearray()
    prev, in_run = None, False
    for k, v in pairs:
        if rle and prev is not None and k == prev:
            out += (b"" if in_run else RLE) + V(len(v)) + v
            in_run = True
        else:
            if in_run:
                out += V_END
                in_run = False
            out += rec(k, v)
        prev = k
    if in_run:
        out += V_END
    return bytes(out + EOF)


def pad_to(body, target, rng):
    """Append whole filler records (state N) until len(body) == target."""
    body = bytearray(body)
    while True:
        r = target - len(body)
        assert r == 0 or r >= 2, "cannot pad to the target"
        if r == 0:
            return body
        size = r
        if r > 120:  # one-byte vints only: a record is 2 + k + v bytes
            size = 100
        k = min(size - 2, 60)
        v = size - 2 - k
        body += rec(bytes(rng.randrange(256) for _ in range(k)),
                    bytes(rng.randrange(256) for _ in range(v)))


# ---- reference and device decode -----------------------------------------
def expected(stream, with_header):
    recs = o.ifile_read(stream, with_header=with_header)
    assert recs == ifile.read_stream(stream, with_header=with_header)
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    klen = np.zeros(len(recs), dtype=np.uint32)
    parts = []
    pos = 0
    for i, (k, v, _same) in enumerate(recs):
        parts += [k, v]
        klen[i] = len(k)
        pos += len(k) + len(v)
        off[i + 1] = pos
    return len(recs), off, klen, b"".join(parts)


def device_decode(engine, stream, with_header=True, verify_crc=True, shift=0):
    """Decode `stream` placed `shift` bytes into a device buffer."""
    dev = engine.upload_bytes(b"\xa5" * shift + stream)
    try:
        d, off, kl, n = engine.ifile_decode(
            ctypes.c_void_p(dev.value + shift), len(stream),
            with_header=with_header, verify_crc=verify_crc)
    finally:
        engine.free_device(dev)
    if n == 0:
        assert d is None and off is None and kl is None
        return 0, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), b""
    h_off = np.frombuffer(engine.read_device(off, 0, 8 * (n + 1)), dtype=np.uint64)
    h_kl = np.frombuffer(engine.read_device(kl, 0, 4 * n), dtype=np.uint32)
    h_data = engine.read_device(d, 0, int(h_off[n]))
    engine.free_device(d, off, kl)
    return n, h_off, h_kl, h_data


def check(engine, stream, with_header=True, shift=0):
    n, off, klen, data = expected(stream, with_header)
    gn, goff, gklen, gdata = device_decode(engine, stream, with_header, with_header,
                                           shift)
    assert gn == n
    assert np.array_equal(goff, off)
    assert np.array_equal(gklen, klen)
    assert gdata == data
    return n


def rc_of(engine, stream, with_header=True, verify_crc=True):
    try:
        device_decode(engine, stream, with_header, verify_crc)
    except engine.EngineError as e:
        return e.rc
    return 0


# ---- 1. hand vectors ------------------------------------------------------
def test_hand_vectors(engine):
    k1, v1 = b"\x00\x00\x00\x01A", b"\x00\x00\x00\x02xy"
    k2, v2 = b"\x00\x00\x00\x01B", b"\x00\x00\x00\x01z"
    plain = bytes([5, 6]) + k1 + v1 + bytes([5, 5]) + k2 + v2 + EOF
    assert check(engine, frame(plain)) == 2
    k = b"\x00\x00\x00\x01K"
    va, vb = b"\x00\x00\x00\x01a", b"\x00\x00\x00\x01b"
    rle = bytes([5, 5]) + k + va + RLE + bytes([5]) + vb + V_END + EOF
    assert check(engine, frame(rle)) == 2
    assert check(engine, rle, with_header=False) == 2
    # bytes after the EOF marker are ignored
    assert check(engine, rle + b"\x07garbage", with_header=False) == 2


def test_empty_segment(engine):
    assert check(engine, frame(EOF)) == 0
    assert check(engine, EOF, with_header=False) == 0


def test_zero_length_key_and_value(engine):
    assert check(engine, frame(rec(b"", b"") + EOF)) == 1
    assert check(engine, frame(rec(b"", b"") + rec(b"k", b"") + rec(b"", b"v") + EOF)) == 3


def test_zero_length_values_in_rle_run(engine):
    # one-byte transitions in state R
    body = rec(b"key", b"") + RLE + b"\x00" + b"\x00" * 40 + V_END + rec(b"z", b"") + EOF
    assert check(engine, frame(body)) == 43
    # a stream that opens with an RLE marker: empty key, as read_stream
    assert check(engine, frame(RLE + V(2) + b"ab" + V(1) + b"c" + V_END + EOF)) == 2


# ---- 2. vint widths -------------------------------------------------------
@pytest.mark.parametrize("ser", [o.serialize_bytes_writable, o.serialize_text])
def test_vint_widths(engine, ser):
    rng = random.Random(11)
    pairs = []
    for ln in (127, 128, 255, 256, 65536):
        pairs.append((ser(bytes(rng.randrange(256) for _ in range(ln))),
                      ser(bytes(rng.randrange(256) for _ in range(ln)))))
        pairs.append((pairs[-1][0], ser(b"same")))
    pairs.append((ser(b"big"), bytes(rng.randrange(256) for _ in range(70000))))
    pairs.append((ser(b"big"), b""))
    assert check(engine, frame(write_body(pairs))) == len(pairs)
    assert check(engine, frame(write_body(pairs, rle=False))) == len(pairs)


# ---- 3. chunk and group edges --------------------------------------------
def _tail(rng):
    return (rec(b"k-own", b"value") + RLE + V(3) + b"abc" + V(0) + V_END
            + rec(b"last", bytes(rng.randrange(256) for _ in range(33))) + EOF)


@pytest.mark.parametrize("delta", [-2, -1, 0, 1])
def test_record_boundary_at_chunk_edge(engine, geom, delta):
    C, _ = geom
    rng = random.Random(100 + delta)
    # delta -1: klen vint at C-1, vlen vint at C (one record's vints split)
    body = bytes(pad_to(b"", C + delta, rng)) + _tail(rng)
    check(engine, frame(body))
    check(engine, body, with_header=False, shift=1)


@pytest.mark.parametrize("delta", [-2, -1])
def test_multibyte_vint_split_across_chunks(engine, geom, delta):
    C, _ = geom
    rng = random.Random(7)
    body = pad_to(b"", C + delta, rng)
    body += rec(bytes(300), bytes(rng.randrange(256) for _ in range(70000)))  # 3B vints
    body += _tail(rng)
    check(engine, frame(bytes(body)))


@pytest.mark.parametrize("at", [-1, 0])
def test_v_end_at_chunk_edge(engine, geom, at):
    C, _ = geom
    rng = random.Random(21)
    run = rec(b"kk", b"v0") + RLE + V(2) + b"v1" + V(5) + b"v2222"
    body = pad_to(b"", 2 * C + at - len(run), rng) + run
    assert len(body) == 2 * C + at
    body += V_END + _tail(rng)
    check(engine, frame(bytes(body)))
    # ... and V_END straight into EOF across the edge
    body2 = pad_to(b"", 2 * C + at - len(run), rng) + run + V_END + EOF
    check(engine, frame(bytes(body2)))


def test_eof_marker_split_across_chunks(engine, geom):
    C, _ = geom
    rng = random.Random(22)
    check(engine, frame(bytes(pad_to(b"", C - 1, rng)) + EOF))
    check(engine, bytes(pad_to(b"", 3 * C - 1, rng)) + EOF, with_header=False)


def test_record_longer_than_a_group(engine, geom):
    C, G = geom
    rng = random.Random(23)
    big = np.random.default_rng(5).integers(0, 256, G * C + 100, dtype=np.uint8).tobytes()
    body = pad_to(b"", C + 17, rng) + rec(b"jump", big) + _tail(rng)
    check(engine, frame(bytes(body)))
    # a same-key record with the long value: the key comes from before the jump
    body = (pad_to(b"", 50, rng) + rec(b"src-key", b"x") + RLE + V(len(big)) + big
            + V(1) + b"y" + V_END + _tail(rng))
    check(engine, frame(bytes(body)))


@pytest.mark.parametrize("which", ["C-1", "C", "C+1", "G*C", "G*C+C+1"])
def test_body_lengths(engine, geom, which):
    C, G = geom
    L = eval(which, {"C": C, "G": G})
    rng = random.Random(24)
    body = bytes(pad_to(b"", L - 2, rng)) + EOF
    assert len(body) == L
    check(engine, frame(body))
    check(engine, body, with_header=False)


def test_rle_run_spanning_three_groups(engine, geom):
    C, G = geom
    rng = random.Random(25)
    body = pad_to(b"", G * C - 500, rng)           # key-bearing record in group 0
    body += rec(b"the-run-key", b"first")
    body += RLE
    while len(body) < 2 * G * C + 3 * C:            # last SAME_KEY record in group 2
        ln = rng.choice([0, 1, 100, 900, 3000])
        body += V(ln) + bytes(rng.randrange(256) for _ in range(ln))
    body += V_END + _tail(rng)
    check(engine, frame(bytes(body)))


# ---- 4. marker-looking payloads ------------------------------------------
def _fill(kind, n, rng):
    if kind == "x80":
        return bytes(0x80 + rng.randrange(16) for _ in range(n))
    if kind == "random":
        return bytes(rng.randrange(256) for _ in range(n))
    return bytes([int(kind, 16)]) * n


@pytest.mark.parametrize("kind", ["ff", "fe", "fd", "x80", "random"])
def test_marker_looking_payloads(engine, geom, kind):
    C, G = geom
    rng = random.Random(zlib.crc32(kind.encode()))
    pairs = []
    size = 0
    lens = [0, 1, 2, 3, 9, 17, 127, 128, 300, 5000]
    while size < 2 * G * C + C:  # counts what RLE framing is sure to keep
        k = _fill(kind, rng.choice(lens[:9]), rng)
        for _ in range(rng.choice([1, 1, 2, 4])):
            v = _fill(kind, rng.choice(lens), rng)
            pairs.append((k, v))
            size += len(v) + 1
    body = write_body(pairs)
    assert len(body) >= 2 * G * C
    assert check(engine, frame(body)) == len(pairs)


# ---- 5. both orders of RLE ------------------------------------------------
@pytest.mark.parametrize("rle_mode", [0, 1])
@pytest.mark.parametrize("shape", ["wordcount", "unique"])
def test_oracle_spill_segments(engine, rle_mode, shape):
    rng = random.Random(31)
    P = 3
    if shape == "wordcount":
        words = [b"w%03d" % i for i in range(40)]
        pairs = [(o.serialize_text(rng.choice(words)), (1).to_bytes(4, "big"))
                 for _ in range(6000)]
    else:
        pairs = [(o.serialize_text(b"u%06d-%s" % (i, b"x" * (i % 13))),
                  i.to_bytes(4, "big")) for i in range(6000)]
        rng.shuffle(pairs)
    d, f, kl = o.build_records(pairs)
    sp = o.spill(d, f, kl, P, key_type=o.KEY_TEXT, comparator=o.CMP_TEXT,
                 rle_mode=rle_mode)
    total = 0
    # the whole spill file on the device; segments sliced with the index
    dev = engine.upload_bytes(sp["data"])
    for st, raw, cl in o.index_decode(sp["index"], P):
        seg = sp["data"][st:st + cl]
        n, off, klen, data = expected(seg, True)
        dd, do, dk, gn = engine.ifile_decode(ctypes.c_void_p(dev.value + st), cl)
        assert gn == n
        if n:
            assert engine.read_device(do, 0, 8 * (n + 1)) == off.tobytes()
            assert engine.read_device(dk, 0, 4 * n) == klen.tobytes()
            assert engine.read_device(dd, 0, len(data)) == data
            engine.free_device(dd, do, dk)
        total += n
    engine.free_device(dev)
    assert total == len(pairs)


# ---- 6. rejections --------------------------------------------------------
def _flip(stream, at, bit=0x10):
    b = bytearray(stream)
    b[at] ^= bit
    return bytes(b)


def _good(rng):
    return frame(bytes(pad_to(b"", 5000, rng)) + _tail(rng))


def _rejections():
    rng = random.Random(41)
    good = _good(rng)
    body = good[4:-4]
    cut = body[:4990]  # the middle of a filler record's bytes
    yield "body bit", _flip(good, 700), -74
    yield "trailer bit", _flip(good, len(good) - 2), -74
    yield "bad magic", b"TIX" + good[3:], -22
    yield "header flag 2", good[:3] + b"\x02" + good[4:], -22
    yield "cut in a key", frame(rec(b"abc", b"de") + V(10) + V(2) + b"12345"), -22
    yield "cut in the body", frame(cut), -22
    yield "klen -5", frame(rec(b"a", b"b") + V(-5) + V(1) + b"xy" + EOF), -22
    yield "vlen too large", frame(rec(b"a", b"b") + V(1) + V(1 << 20) + b"k" + EOF), -22
    yield "no EOF marker", frame(rec(b"a", b"b") + rec(b"c", b"d")), -22
    yield "vint past the end", frame(rec(b"a", b"b") + V(1) + b"\x8c\x01"), -22
    yield "9-byte vint, huge", frame(rec(b"a", b"b") + b"\x88" + b"\xff" * 8 + V(1) + EOF), -22
    yield "negative 9-byte vint", frame(rec(b"a", b"b") + b"\x80" + b"\xff" * 8 + V(1) + EOF), -22
    yield "vlen -1 after a key", frame(V(1) + V(-1) + b"k" + EOF), -22
    yield "V_END as klen", frame(rec(b"a", b"b") + V_END + V(1) + b"x" + EOF), -22
    yield "EOF inside an RLE run", frame(rec(b"a", b"b") + RLE + V(1) + b"x" + EOF), -22


@pytest.mark.parametrize("name,stream,want", list(_rejections()),
                         ids=[r[0] for r in _rejections()])
def test_rejections(engine, name, stream, want):
    with pytest.raises(Exception):
        ifile.read_stream(stream)
    assert rc_of(engine, stream) == want
    # the engine is still usable afterwards
    assert check(engine, _good(random.Random(42))) > 0


def test_compressed_flag_is_refused_by_the_device(engine):
    good = _good(random.Random(43))
    tif1 = ifile.compress_segment(good)
    assert rc_of(engine, tif1) == -22
    assert rc_of(engine, _flip(tif1, 9)) == -74  # CRC below the codec comes first


# ---- 7. merge end to end --------------------------------------------------
def _unique_pairs(n, seed):
    rng = random.Random(seed)
    seen = set()
    out = []
    while len(out) < n:
        k = bytes(rng.randrange(256) for _ in range(10))
        if k in seen:
            continue
        seen.add(k)
        out.append((o.serialize_bytes_writable(k),
                    o.serialize_bytes_writable(bytes(rng.randrange(256)
                                                     for _ in range(rng.randrange(1, 40))))))
    return out


@pytest.mark.parametrize("K", [1, 3, 17])
def test_merge_ifile_segments_single_partition(engine, K):
    pairs = _unique_pairs(K * 300, seed=50 + K)
    spills = []
    s = engine.Sorter(engine.make_conf(1))
    for i in range(K):
        d, f, kl = o.build_records(pairs[i * 300:(i + 1) * 300])
        sp = o.spill(d, f, kl, 1)
        spills.append(sp)
        dev = engine.upload_bytes(sp["data"])
        s.add_ifile_segment(dev, len(sp["data"]), partition=-1)
        engine.free_device(dev)  # the sorter keeps its own decoded copy
    s.flush()
    got, gidx = s.output()
    s.close()
    want = o.final_merge(spills, 1)
    assert gidx == o.index_decode(want["index"], 1)
    assert got == want["data"]


def test_merge_ifile_segments_explicit_partitions(engine):
    P, K = 4, 5
    pairs = _unique_pairs(K * 400, seed=61)
    spills = []
    s = engine.Sorter(engine.make_conf(P))
    for i in range(K):
        batch = pairs[i * 400:(i + 1) * 400]
        d, f, kl = o.build_records(batch)
        # range placement on the leading content byte: not the hash placement
        parts = np.array([k[4] * P // 256 for k, _ in batch], dtype=np.int32)
        sp = o.spill(d, f, kl, P, partitions=parts)
        spills.append(sp)
        dev = engine.upload_bytes(sp["data"])
        for p, (st, raw, cl) in enumerate(o.index_decode(sp["index"], P)):
            s.add_ifile_segment(ctypes.c_void_p(dev.value + st), cl, partition=p)
        engine.free_device(dev)
    s.flush()
    got, gidx = s.output()
    s.close()
    want = o.final_merge(spills, P)
    assert gidx == o.index_decode(want["index"], P)
    assert got == want["data"]


def test_add_ifile_segment_refuses_buffered_writes_and_bad_partition(engine):
    stream = frame(rec(o.serialize_bytes_writable(b"k"), o.serialize_bytes_writable(b"v"))
                   + EOF)
    dev = engine.upload_bytes(stream)
    s = engine.Sorter(engine.make_conf(2))
    with pytest.raises(engine.EngineError) as e:
        s.add_ifile_segment(dev, len(stream), partition=2)
    assert e.value.rc == -22
    s.write(o.serialize_bytes_writable(b"a"), o.serialize_bytes_writable(b"b"), -1)
    with pytest.raises(engine.EngineError, match="buffered writes") as e:
        s.add_ifile_segment(dev, len(stream), partition=-1)
    assert e.value.rc == -22
    s.close()
    engine.free_device(dev)


def test_add_ifile_segment_rejects_unsorted(engine):
    pairs = _unique_pairs(200, seed=71)  # random order
    stream = frame(write_body(pairs))
    dev = engine.upload_bytes(stream)
    s = engine.Sorter(engine.make_conf(1))
    with pytest.raises(engine.EngineError, match="not sorted") as e:
        s.add_ifile_segment(dev, len(stream))
    assert e.value.rc == -22
    s.close()
    engine.free_device(dev)


# ---- 8. reference bytes ---------------------------------------------------
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                       "TestIFile_concatenated_compressed.bin")
COMPRESSED = [723, 25396, 10926, 8203, 6665]


def test_reference_fixture_payloads(engine):
    blob = open(FIXTURE, "rb").read()
    pos = 0
    for comp_len in COMPRESSED:
        seg = blob[pos:pos + comp_len]
        pos += comp_len
        payload = zlib.decompress(seg[4:-4])
        want = o.ifile_read(payload, with_header=False)
        n, off, klen, data = device_decode(engine, payload, with_header=False)
        assert n == len(want) > 0
        got = [(data[int(off[i]):int(off[i]) + int(klen[i])],
                data[int(off[i]) + int(klen[i]):int(off[i + 1])]) for i in range(n)]
        assert got == [(k, v) for k, v, _ in want]
        for k, v in got:
            assert len(v) == 4
            ln, sz = o.vint_decode(k)
            assert sz + ln == len(k)
        check(engine, payload, with_header=False)


# ---- 9. plugin ------------------------------------------------------------
WORDS = ("the quick brown fox jumps over lazy dog alpha beta gamma delta "
         "epsilon zeta eta theta").split()


@pytest.mark.parametrize("compressed", [False, True])
def test_plugin_wordcount_never_touches_the_host_write_path(engine, monkeypatch,
                                                            compressed):
    from tez_amd.ordered_output import OrderedPartitionedKVOutput
    from tez_amd.ordered_input import OrderedGroupedKVInput

    P = 3
    props = {"tez.runtime.key.class": "org.apache.hadoop.io.Text",
             "tez.runtime.value.class": "org.apache.hadoop.io.IntWritable"}
    rng = random.Random(9)
    docs = [[WORDS[rng.randrange(len(WORDS))] for _ in range(3000)] for _ in range(2)]
    outputs = []
    for m, doc in enumerate(docs):
        out = OrderedPartitionedKVOutput(P, props, unique_id=f"attempt_d{m}").start()
        w = out.get_writer()
        for word in doc:
            w.write(word.encode(), 1)
        out.close()
        outputs.append(out)

    def boom(self, *a, **kw):
        raise AssertionError("reduce side went through Sorter.write")
    monkeypatch.setattr(engine.Sorter, "write", boom)

    counted = {}
    for p in range(P):
        inp = OrderedGroupedKVInput(p, props)
        for out in outputs:
            seg, _raw = out.segment(p)
            if compressed and len(seg):
                seg = ifile.compress_segment(seg)
            inp.add_segment(seg)
        inp.start()
        for key, vals in inp.get_reader():
            assert key.decode() not in counted
            counted[key.decode()] = sum(int.from_bytes(v, "big") for v in vals)
    assert counted == dict(collections.Counter(w for doc in docs for w in doc))
