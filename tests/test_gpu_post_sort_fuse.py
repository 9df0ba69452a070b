"""Post-sort metadata kernel (k_post_sort_meta), the tile skip in
k_refine_compact_lb, and the CRC fold: one CRC per 4 KiB unit out of
k_crc_chunks (four units, one per wave, to a 16 KiB super-chunk), folded per
range by k_crc_combine_ranges.

Every case compares the IFile stream and the index byte for byte with the
CPU oracle.  The metadata kernel and the tile skip are the only path: the
separate passes they replaced, and the switch that selected them, are gone.

Shapes sit on the edges of SCAN_TILE = 2048 positions, of the 4096-byte CRC
unit and of the 16384-byte CRC super-chunk."""
import random

import numpy as np
import pytest

import oracle as o

pytestmark = pytest.mark.gpu

TILE = 2048
SC_BYTES = 16384
UNIT_BYTES = 4096


@pytest.fixture(scope="module")
def engine():
    import __graft_entry__
    __graft_entry__.build()
    import tez_amd
    if not tez_amd.device_available():
        pytest.skip("no GPU")
    return tez_amd


def _records_from_keys(keys, vlen, seed):
    """BytesWritable records over an (n, klen) uint8 key matrix, random
    values, columnar."""
    rng = np.random.default_rng(seed)
    n, klen = keys.shape
    rec = 8 + klen + vlen
    m = np.zeros((n, rec), dtype=np.uint8)
    m[:, 0:4] = np.frombuffer(int(klen).to_bytes(4, "big"), dtype=np.uint8)
    m[:, 4:4 + klen] = keys
    m[:, 4 + klen:8 + klen] = np.frombuffer(int(vlen).to_bytes(4, "big"),
                                            dtype=np.uint8)
    m[:, 8 + klen:] = rng.integers(0, 256, size=(n, vlen), dtype=np.uint8)
    data = m.reshape(-1).copy()
    offs = np.arange(0, rec * (n + 1), rec, dtype=np.uint64)
    klens = np.full(n, 4 + klen, dtype=np.uint32)
    return data, offs, klens


def _unique_keys(n, klen, seed):
    """(n, klen) keys, unique in their first 4 bytes, random order."""
    rng = np.random.default_rng(seed)
    ids = rng.choice(2 ** 31, size=n, replace=False)
    keys = rng.integers(0, 256, size=(n, klen), dtype=np.uint8)
    for b in range(4):
        keys[:, b] = (ids >> (8 * (3 - b))) & 0xFF
    return keys


def _be_prefix(keys, values, nbytes):
    """Write `values` big-endian into the first nbytes key bytes."""
    for b in range(nbytes):
        keys[:, b] = (values >> (8 * (nbytes - 1 - b))) & 0xFF


def _sort_uploaded(engine, data, offs, klens, P, parts=None, **conf_kw):
    d, doff, dkl, dpart = engine.upload_records(bytes(data), offs, klens, parts)
    s = engine.Sorter(engine.make_conf(P, **conf_kw))
    s.write_batch_device(d, doff, dkl, dpart, len(klens))
    s.flush()
    got = s.output()
    s.close()
    engine.free_device(d, doff, dkl, dpart)
    return got


def _check(engine, data, offs, klens, P, parts=None):
    want = o.spill(data, offs, klens, P, key_type=o.KEY_BYTES,
                   comparator=o.CMP_TEZBYTES, partitions=parts)
    want_index = o.index_decode(want["index"], P)
    got, gidx = _sort_uploaded(engine, data, offs, klens, P, parts)
    assert gidx == want_index, "index"
    assert got == want["data"], "stream"
    return want, want_index


# ---- tile edges and partition starts -------------------------------------

@pytest.mark.parametrize("n", [1, 2, 2047, 2048, 2049, 4097])
def test_tile_edges(engine, n):
    """P=64, 88-byte records.  n = 1 and 2 leave nearly every partition
    empty (leading, trailing and interior gaps in the partition starts); the
    others put the last position just inside, on and just past a tile."""
    data, offs, klens = _records_from_keys(_unique_keys(n, 16, 300 + n), 64,
                                           seed=400 + n)
    _check(engine, data, offs, klens, 64)


@pytest.mark.parametrize("P", [1, 2, 3, 199])
def test_partition_counts(engine, P):
    """P=1 has no partition bits in the composite; 3 and 199 are no powers
    of two (199 > the records of some tiles' partitions: empty ones occur)."""
    n = 3001
    data, offs, klens = _records_from_keys(_unique_keys(n, 16, 500 + P), 64,
                                           seed=600 + P)
    _check(engine, data, offs, klens, P)


def _explicit_parts(kind, n):
    if kind == "all_last":
        return np.full(n, 15, dtype=np.int32)
    if kind == "all_first":
        return np.zeros(n, dtype=np.int32)
    if kind == "first_and_last":
        return np.where(np.arange(n) % 3 == 0, 0, 15).astype(np.int32)
    assert kind == "boundary_on_tile_edge"
    parts = np.ones(n, dtype=np.int32)
    parts[np.random.default_rng(5).permutation(n)[:TILE]] = 0
    assert int((parts == 0).sum()) == TILE
    return parts


@pytest.mark.parametrize("kind", ["all_last", "all_first", "first_and_last",
                                  "boundary_on_tile_edge"])
def test_explicit_partitions(engine, kind):
    """n = 4101, P = 16, caller-supplied partitions: every record in the
    last partition (15 leading empties), in the first (15 trailing), only in
    0 and 15 (14 interior empties filled from one position), and a 0/1
    boundary that sits exactly on a tile edge."""
    n, P = 4101, 16
    data, offs, klens = _records_from_keys(_unique_keys(n, 16, 700), 64,
                                           seed=701)
    _check(engine, data, offs, klens, P,
                      _explicit_parts(kind, n))


# ---- ties, tile skip, refinement levels ----------------------------------

def test_equal_run_across_tile_edge(engine):
    """P=1, n=4100: key i is the integer i, except that 2040..2055 all carry
    2040, so one run of 16 fully equal keys occupies sorted positions
    2040..2055 over the first tile edge (eq lookahead and in-run counts on
    both tiles; 15 equal pairs stay below the writer-RLE gate)."""
    n = 4100
    ids = np.arange(n, dtype=np.int64)
    ids[2040:2056] = 2040
    keys = np.zeros((n, 16), dtype=np.uint8)
    _be_prefix(keys, ids, 4)
    keys = keys[np.random.default_rng(9).permutation(n)]
    data, offs, klens = _records_from_keys(keys, 64, seed=10)
    want, _ = _check(engine, data, offs, klens, 1)
    assert want["rle"] == 0


def test_equal_pairs_turn_writer_rle_on(engine):
    """P=1, n=4100, every key twice: 2050 equal pairs, well over a tenth of
    n, so the eq count that now comes from the metadata kernel must switch
    the writer's RLE on."""
    n = 4100
    keys = np.zeros((n, 16), dtype=np.uint8)
    _be_prefix(keys, np.arange(n, dtype=np.int64) // 2 * 7919, 4)
    keys = keys[np.random.default_rng(11).permutation(n)]
    data, offs, klens = _records_from_keys(keys, 64, seed=12)
    want, _ = _check(engine, data, offs, klens, 1)
    assert want["rle"] == 1


def test_skipped_tiles_between_live_ones(engine):
    """P=1, n = 3*2048 + 56: the composite covers the first 3 key bytes at
    this n.  Only the 5 smallest and the 6 largest keys share those bytes
    (two of the largest are fully equal); every key between is alone.  Tile
    0 and the last tile compact, the tiles between publish nothing, and the
    last tile's slots continue after tile 0's."""
    n = 3 * TILE + 56
    rng = np.random.default_rng(21)
    keys = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    mid = rng.choice(np.arange(1, 2 ** 24 - 1), size=n - 11, replace=False)
    pref = np.concatenate([np.zeros(5, dtype=np.int64), mid,
                           np.full(6, 2 ** 24 - 1, dtype=np.int64)])
    _be_prefix(keys, pref, 3)
    keys[n - 1] = keys[n - 2]
    keys = keys[rng.permutation(n)]
    data, offs, klens = _records_from_keys(keys, 64, seed=22)
    _check(engine, data, offs, klens, 1)


def test_multi_level_refinement(engine):
    """P=1, 16-byte keys.  Groups of 4 share their first 12 bytes and differ
    in the last 4, so they survive level 0 (bytes 3..10) and split at level
    1; in every sixth group two keys are fully equal and go on to the length
    level.  The groups hold the smallest prefixes and one the largest, every
    other key is alone in its first 3 bytes: the level-0 tile counts (first
    and last tile live, the rest empty) must still hold at levels 1 and 2."""
    rng = np.random.default_rng(31)
    ngroups, nsingle = 61, 4500
    gkeys = np.zeros((ngroups * 4, 16), dtype=np.uint8)
    gpref = np.sort(rng.choice(2 ** 20, size=ngroups, replace=False))
    gpref[-1] = 2 ** 24 - 1
    for g in range(ngroups):
        body = rng.integers(0, 256, size=12, dtype=np.uint8)
        gkeys[4 * g:4 * g + 4, :12] = body
        gkeys[4 * g:4 * g + 4, 12:] = rng.integers(0, 256, size=(4, 4),
                                                   dtype=np.uint8)
        gkeys[4 * g:4 * g + 4, 15] = np.arange(4)  # distinct within group
        if g % 6 == 0:
            gkeys[4 * g + 3] = gkeys[4 * g + 2]
    _be_prefix(gkeys, np.repeat(gpref, 4), 3)
    skeys = rng.integers(0, 256, size=(nsingle, 16), dtype=np.uint8)
    _be_prefix(skeys, rng.choice(np.arange(2 ** 22, 2 ** 24 - 1), size=nsingle,
                                 replace=False), 3)
    keys = np.concatenate([gkeys, skeys])
    keys = keys[rng.permutation(len(keys))]
    data, offs, klens = _records_from_keys(keys, 24, seed=32)
    _check(engine, data, offs, klens, 1)


# ---- merge entry (lo keys given) -----------------------------------------

@pytest.mark.parametrize("sizes", [(1000, 1100), (1500, 1500, 1150)])
def test_merge_entry(engine, sizes):
    """Two and three spills, then flush, P=4: the merge hands the lo keys
    to the metadata kernel.  Keys repeat within and across spills; the
    totals (2100, 4150) straddle one and two tiles."""
    P = 4
    rng = random.Random(41 + len(sizes))
    pool = [o.serialize_bytes_writable(b"mk%06d-pad-pad" % i)
            for i in range(sum(sizes) // 2)]
    batches = []
    for si, cnt in enumerate(sizes):
        batches.append([(pool[rng.randrange(len(pool))],
                         o.serialize_bytes_writable(b"s%dv%05d" % (si, j)))
                        for j in range(cnt)])
    spills = []
    for batch in batches:
        d, f, kl = o.build_records(batch)
        spills.append(o.spill(d, f, kl, P))
    want = o.final_merge(spills, P)
    want_index = o.index_decode(want["index"], P)
    s = engine.Sorter(engine.make_conf(P, key_type=engine.KEY_BYTES,
                                       comparator=engine.CMP_TEZBYTES))
    for batch in batches:
        for k, v in batch:
            s.write(k, v, -1)
        s.spill()
    assert s.num_spills() == len(sizes)
    s.flush()
    got, gidx = s.output()
    s.close()
    assert gidx == want_index, "index"
    assert got == want["data"], "stream"


# ---- combiner: partition counts after the view was replaced --------------

def test_combiner_single_spill(engine):
    """SUM_INT combiner: the fold replaces n and the partition array, so the
    partition counts come from k_part_hist, not from the starts taken before
    the fold."""
    P = 8
    rng = random.Random(51)
    keys = [b"key%04d" % i for i in range(61)]
    pairs = [(o.serialize_text(keys[rng.randrange(61)]),
              int(rng.randrange(-100, 1000)).to_bytes(4, "big", signed=True))
             for _ in range(5000)]
    d, f, kl = o.build_records(pairs)
    want = o.spill(d, f, kl, P, key_type=o.KEY_TEXT, comparator=o.CMP_TEXT,
                   combiner=1)
    want_index = o.index_decode(want["index"], P)
    s = engine.Sorter(engine.make_conf(P, key_type=engine.KEY_TEXT,
                                       comparator=engine.CMP_TEXT,
                                       combiner=1))
    for k, v in pairs:
        s.write(k, v, -1)
    s.flush()
    got, gidx = s.output()
    s.close()
    assert gidx == want_index, "index"
    assert got == want["data"], "stream"


# ---- CRC lengths and byte phases -----------------------------------------

def _two_size_records(n15, n16):
    """n15 records that take 15 IFile bytes and n16 that take 16 (4-byte
    unique keys, 1- or 2-byte values; two 1-byte length vints each)."""
    pairs = []
    for i in range(n15 + n16):
        v = b"x" if i < n15 else b"yz"
        pairs.append((o.serialize_bytes_writable(int(i).to_bytes(4, "big")),
                      o.serialize_bytes_writable(v)))
    random.Random(61).shuffle(pairs)
    return o.build_records(pairs)


@pytest.mark.parametrize("L", [47, 256, UNIT_BYTES - 1, UNIT_BYTES,
                               UNIT_BYTES + 1, 2 * UNIT_BYTES, 3 * UNIT_BYTES,
                               SC_BYTES - 1, SC_BYTES, SC_BYTES + 1,
                               2 * SC_BYTES + 255])
def test_crc_lengths(engine, L):
    """One partition whose checksummed length (records + 2 EOF bytes) is L:
    below one chunk, exactly one chunk, one byte short of / exactly / one
    byte past a 4 KiB unit, exactly two and three units (the range ends
    where wave 2 / wave 3 of the block would start), one byte short of /
    exactly / one byte past a super-chunk, and two super-chunks plus a
    ragged chunk of 255.  15a + 16b = L - 2 with b = (L - 2) mod 15."""
    b = (L - 2) % 15
    a = (L - 2 - 16 * b) // 15
    assert a >= 0 and 15 * a + 16 * b == L - 2
    data, offs, klens = _two_size_records(a, b)
    want = o.spill(data, offs, klens, 1, key_type=o.KEY_BYTES,
                   comparator=o.CMP_TEZBYTES)
    want_index = o.index_decode(want["index"], 1)
    # raw length = 4-byte header + checksummed range
    assert want_index[0][1] - 4 == L, "shape drifted: intended L not hit"
    got, gidx = _sort_uploaded(engine, data, offs, klens, 1)
    assert gidx == want_index
    assert got == want["data"]


def test_crc_range_start_phases(engine):
    """8 partitions of 1200 + p fifteen-byte records: every range is longer
    than a super-chunk (full chunks take the funnel-shift loads) and the
    range starts fall on all four byte phases."""
    P = 8
    counts = [1200 + p for p in range(P)]
    n = sum(counts)
    pairs = [(o.serialize_bytes_writable(int(i).to_bytes(4, "big")),
              o.serialize_bytes_writable(b"x")) for i in range(n)]
    parts = np.repeat(np.arange(P, dtype=np.int32), counts)
    perm = np.random.default_rng(71).permutation(n)
    pairs = [pairs[i] for i in perm]
    parts = parts[perm].copy()
    data, offs, klens = o.build_records(pairs)
    want = o.spill(data, offs, klens, P, key_type=o.KEY_BYTES,
                   comparator=o.CMP_TEZBYTES, partitions=parts)
    want_index = o.index_decode(want["index"], P)
    assert {(st + 4) % 4 for st, _raw, _cl in want_index} == {0, 1, 2, 3}, \
        "shape drifted: not every start phase occurs"
    assert all(raw - 4 > SC_BYTES for _st, raw, _cl in want_index)
    got, gidx = _sort_uploaded(engine, data, offs, klens, P, parts)
    assert gidx == want_index
    assert got == want["data"]


@pytest.mark.parametrize("n", [11700, 23400])
def test_crc_range_over_256_units(engine, n):
    """One partition of n records that take 90 IFile bytes each: 258 and 515
    units with a short last one, so every thread of the range's combine block
    folds a span of 2 (4) units with the shift-by-4096 table before the
    tree."""
    data, offs, klens = _records_from_keys(_unique_keys(n, 16, 80 + n), 64,
                                           seed=81)
    want = o.spill(data, offs, klens, 1, key_type=o.KEY_BYTES,
                   comparator=o.CMP_TEZBYTES)
    want_index = o.index_decode(want["index"], 1)
    L = want_index[0][1] - 4
    assert L == 90 * n + 2, "shape drifted"
    units = -(-L // UNIT_BYTES)
    assert units > 256 * (n // 11700) and L % UNIT_BYTES != 0
    got, gidx = _sort_uploaded(engine, data, offs, klens, 1)
    assert gidx == want_index
    assert got == want["data"]


# ---- the benchmark's route -----------------------------------------------

def test_adopted_generated_batch(engine):
    """Device-generated 88-byte records handed over with
    write_batch_device_adopt, n = 300,000 and P = 64: about 150 tiles and
    about 25 super-chunks per partition."""
    from tez_amd._engine import lib, _ck
    n, P, klen, vlen = 300_000, 64, 16, 64
    rec = 8 + klen + vlen
    conf = engine.make_conf(P)
    d, off, kl, part = engine.generate(seed=0xF05E, n=n, kind=0, klen=klen,
                                       vlen=vlen, conf=conf)
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
    assert gidx == want_index, "index"
    assert got == want["data"], "stream"
