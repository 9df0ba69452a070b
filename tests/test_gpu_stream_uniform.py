"""Streamed uniform-record composite build (k_build_composite_stream):
single-spill, BYTES-key, uniform records of a whole number of dwords up to
128 bytes.  Every case sorts the same unique-key records twice, once on the
default path and once with TZS_STREAM_UNIFORM=0 (k_build_composite2), and
both IFile streams and indexes must equal the CPU oracle byte for byte, and
hence each other."""
import numpy as np
import pytest

import oracle as o

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import __graft_entry__
    __graft_entry__.build()
    import tez_amd
    if not tez_amd.device_available():
        pytest.skip("no GPU")
    return tez_amd


def _records(n, klen, vlen, seed):
    """n BytesWritable key/value records with unique keys, columnar."""
    rng = np.random.default_rng(seed)
    rec = 8 + klen + vlen
    m = np.zeros((n, rec), dtype=np.uint8)
    m[:, 0:4] = np.frombuffer(int(klen).to_bytes(4, "big"), dtype=np.uint8)
    # unique keys: distinct integers below 256**min(klen, 4), big-endian, in
    # the leading key bytes; the remaining key bytes are random
    kb = min(klen, 4)
    ids = rng.choice(256 ** kb if kb < 4 else 2 ** 31, size=n, replace=False)
    for b in range(kb):
        m[:, 4 + b] = (ids >> (8 * (kb - 1 - b))) & 0xFF
    if klen > kb:
        m[:, 4 + kb:4 + klen] = rng.integers(0, 256, size=(n, klen - kb),
                                             dtype=np.uint8)
    m[:, 4 + klen:8 + klen] = np.frombuffer(int(vlen).to_bytes(4, "big"),
                                            dtype=np.uint8)
    m[:, 8 + klen:] = rng.integers(0, 256, size=(n, vlen), dtype=np.uint8)
    data = m.reshape(-1).copy()
    offs = np.arange(0, rec * (n + 1), rec, dtype=np.uint64)
    klens = np.full(n, 4 + klen, dtype=np.uint32)
    return data, offs, klens


def _sort_uploaded(engine, data, offs, klens, P, parts=None):
    d, doff, dkl, dpart = engine.upload_records(bytes(data), offs, klens, parts)
    s = engine.Sorter(engine.make_conf(P))
    s.write_batch_device(d, doff, dkl, dpart, len(klens))
    s.flush()
    got = s.output()
    s.close()
    engine.free_device(d, doff, dkl, dpart)
    return got


def _check_both_paths(engine, monkeypatch, data, offs, klens, P, parts=None):
    want = o.spill(data, offs, klens, P, key_type=o.KEY_BYTES,
                   comparator=o.CMP_TEZBYTES, partitions=parts)
    want_index = o.index_decode(want["index"], P)
    for toggle in (None, "0"):
        if toggle is None:
            monkeypatch.delenv("TZS_STREAM_UNIFORM", raising=False)
        else:
            monkeypatch.setenv("TZS_STREAM_UNIFORM", toggle)
        got, gidx = _sort_uploaded(engine, data, offs, klens, P, parts)
        assert gidx == want_index, f"index, TZS_STREAM_UNIFORM={toggle}"
        assert got == want["data"], f"stream, TZS_STREAM_UNIFORM={toggle}"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 4113])
def test_tail_and_partition_boundaries(engine, monkeypatch, n):
    """rec 88 (22 dwords), 64 partitions: no full 64-record wave, exactly
    one, one plus a tail, and many waves plus a tail (4113 = 64*64 + 17)."""
    data, offs, klens = _records(n, 16, 64, seed=100 + n)
    _check_both_paths(engine, monkeypatch, data, offs, klens, 64)


@pytest.mark.parametrize("P,n", [(1, 64 * 5 + 3), (2, 1000)])
def test_one_and_two_partitions(engine, monkeypatch, P, n):
    """rec 88 with one partition (no partition bits in the composite) and
    with two: full waves, then a tail."""
    data, offs, klens = _records(n, 16, 64, seed=200 + P)
    _check_both_paths(engine, monkeypatch, data, offs, klens, P)


def test_w27_word_count_not_multiple_of_four(engine, monkeypatch):
    """rec 108 (27 dwords, the 10 B key + 90 B value shape): the last
    16-byte streamed load of a run is partial."""
    data, offs, klens = _records(777, 10, 90, seed=27)
    _check_both_paths(engine, monkeypatch, data, offs, klens, 3)


def test_short_content_zero_padded(engine, monkeypatch):
    """rec 12 (3 dwords): 3 content bytes, zero-padded in the composite, and
    a hash over 3 bytes."""
    data, offs, klens = _records(500, 3, 1, seed=3)
    _check_both_paths(engine, monkeypatch, data, offs, klens, 4)


@pytest.mark.parametrize("klen,vlen", [(5, 6), (16, 200)])
def test_outside_the_gate(engine, monkeypatch, klen, vlen):
    """rec 19 (not whole dwords) and rec 228 (> 128): k_build_composite2
    runs whatever the switch says, and still matches."""
    data, offs, klens = _records(900, klen, vlen, seed=klen)
    _check_both_paths(engine, monkeypatch, data, offs, klens, 8)


def test_explicit_partitions_skewed(engine, monkeypatch):
    """rec 88 with a caller-supplied partition array (the hash is skipped):
    most records in one partition, the rest spread thin."""
    n, P = 3000, 16
    data, offs, klens = _records(n, 16, 64, seed=88)
    rng = np.random.default_rng(89)
    parts = np.where(rng.random(n) < 0.85, 5,
                     rng.integers(0, P, size=n)).astype(np.int32)
    _check_both_paths(engine, monkeypatch, data, offs, klens, P, parts)


def test_adopted_generated_batch(engine, monkeypatch):
    """The benchmark's own route: device-generated records handed over with
    write_batch_device_adopt (uniformity known from the generator's hint)."""
    from tez_amd._engine import lib, _ck
    n, P, klen, vlen = 5000, 64, 16, 64
    rec = 8 + klen + vlen
    conf = engine.make_conf(P)
    want = want_index = None
    for toggle in (None, "0"):
        if toggle is None:
            monkeypatch.delenv("TZS_STREAM_UNIFORM", raising=False)
        else:
            monkeypatch.setenv("TZS_STREAM_UNIFORM", toggle)
        d, off, kl, part = engine.generate(seed=0x5EED, n=n, kind=0, klen=klen,
                                           vlen=vlen, conf=conf)
        if want is None:
            data = np.zeros(rec * n, dtype=np.uint8)
            _ck(lib().tzs_memcpy_d2h(data.ctypes.data, d, rec * n), "d2h")
            offs = np.arange(0, rec * (n + 1), rec, dtype=np.uint64)
            klens = np.full(n, 4 + klen, dtype=np.uint32)
            want = o.spill(data, offs, klens, P, key_type=o.KEY_BYTES,
                           comparator=o.CMP_TEZBYTES)
            want_index = o.index_decode(want["index"], P)
        engine.free_device(part)
        s = engine.Sorter(conf)
        s.write_batch_device_adopt(d, off, kl, None, n)
        s.flush()
        got, gidx = s.output()
        s.close()
        assert gidx == want_index, f"index, TZS_STREAM_UNIFORM={toggle}"
        assert got == want["data"], f"stream, TZS_STREAM_UNIFORM={toggle}"
