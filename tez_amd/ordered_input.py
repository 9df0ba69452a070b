"""OrderedGroupedKVInput — the reduce-side plugin surface
(input/OrderedGroupedKVInput.java:101-318) over the HIP engine.

Segments for THIS input's partition are added from producer outputs (the
local DISK_DIRECT path, FetcherOrderedGrouped.java:193-205, or the xGMI
exchange); start() runs the merge (Shuffle.run -> MergeManager.finalMerge
equivalents) and takes the key groups of the merged records from the device
(tzs_sorter_grouped); get_reader() yields
(key_content, [value_content...]) groups with ValuesIterator semantics
(ValuesIterator.java:177-199: same group iff the merge reported SAME_KEY or
the comparator says equal).
"""
import gc
import zlib

import numpy as np

from . import _engine, ifile


class GroupedKV:
    """Host copy of a grouped view: group g owns records
    group_off[g]..group_off[g+1]; its serialized key is
    key_data[key_off[g]:key_off[g+1]]; record i's serialized value is
    val_data[val_off[i]:val_off[i+1]].  Iteration yields
    (deserialized key content, [serialized values]) per group."""

    def __init__(self, key_data, key_off, val_data, val_off, group_off,
                 text_keys=False):
        self.key_data = np.asarray(key_data, dtype=np.uint8)
        self.key_off = np.asarray(key_off, dtype=np.uint64)
        self.val_data = np.asarray(val_data, dtype=np.uint8)
        self.val_off = np.asarray(val_off, dtype=np.uint64)
        self.group_off = np.asarray(group_off, dtype=np.uint64)
        self.text_keys = bool(text_keys)

    def __len__(self):
        return max(len(self.group_off) - 1, 0)

    def key(self, g):
        """Serialized key of group g."""
        if not 0 <= g < len(self):
            raise IndexError(g)
        return self.key_data[int(self.key_off[g]):int(self.key_off[g + 1])].tobytes()

    def values(self, g):
        """Serialized values of group g, in merged order."""
        if not 0 <= g < len(self):
            raise IndexError(g)
        vo = self.val_off
        return [self.val_data[int(vo[i]):int(vo[i + 1])].tobytes()
                for i in range(int(self.group_off[g]), int(self.group_off[g + 1]))]

    @staticmethod
    def _text_skip(first):
        """Bytes of the vint length prefix, from its first byte."""
        s = first - 256 if first >= 128 else first
        if s >= -112:
            return 1
        return (-119 - s) if s < -120 else (-111 - s)

    def _build(self):
        ng = len(self)
        if ng == 0:
            return []
        kb = self.key_data.tobytes()
        vb = self.val_data.tobytes()
        ko = self.key_off.tolist()
        vo = self.val_off.tolist()
        go = self.group_off.tolist()
        if self.text_keys:
            skip = self._text_skip
            keys = [kb[a + (1 if kb[a] < 128 else skip(kb[a])):b]
                    for a, b in zip(ko, ko[1:])]
        else:
            keys = [kb[a + 4:b] for a, b in zip(ko, ko[1:])]
        vals = [vb[a:b] for a, b in zip(vo, vo[1:])]
        if ng == len(vals):  # every group holds one record
            return [(k, [v]) for k, v in zip(keys, vals)]
        return [(k, vals[a:b]) for k, a, b in zip(keys, go, go[1:])]

    def to_list(self):
        """[(deserialized key content, [serialized values])], one entry per
        group, sliced out of the arrays group by group.  The cyclic collector
        is paused while the list is built: bytes, lists and tuples of bytes
        form no cycles, and its generation scans over a few hundred thousand
        fresh containers cost twice the slicing itself (measured, DESIGN.md
        §4d)."""
        was_enabled = gc.isenabled()
        gc.disable()
        try:
            return self._build()
        finally:
            if was_enabled:
                gc.enable()

    def __iter__(self):
        return iter(self.to_list())


class OrderedGroupedKVInput:
    def __init__(self, partition, props=None):
        self.partition = partition
        self.props = dict(props or {})
        self._segments = []
        self._sorter = None
        self._grouped = None
        key_cls = self.props.get("tez.runtime.key.class",
                                 "org.apache.hadoop.io.BytesWritable")
        self._text_keys = key_cls == "org.apache.hadoop.io.Text"

    def add_segment(self, ifile_bytes, raw_length=None):
        """A fetched segment: IFile stream bytes of this partition from one
        producer (ShuffleHeader-framed on the wire; the frame is handled by
        the exchange layer)."""
        if len(ifile_bytes) == 0:
            return
        self._segments.append(ifile_bytes)

    @staticmethod
    def _device_payload(seg):
        """(bytes to upload, with_header) for one fetched segment.  A TIF\\1
        segment has its CRC (over the compressed payload, IFile.java:352-368)
        checked and is inflated here; the device decodes the bare payload.
        Everything else, bad magic included, is judged by the device reader."""
        if len(seg) >= 8 and bytes(seg[:4]) == b"TIF\x01":
            body = bytes(seg[4:-4])
            if zlib.crc32(body) != int.from_bytes(seg[-4:], "big"):
                raise ValueError("IFile CRC mismatch")
            return zlib.decompress(body), False
        return bytes(seg), True

    def _conf(self):
        return _engine.make_conf(
            1,  # single-partition merge; placement already decided map-side
            key_type=_engine.KEY_TEXT if self._text_keys else _engine.KEY_BYTES,
            comparator=_engine.CMP_TEXT if self._text_keys else _engine.CMP_TEZBYTES)

    def _merge_sorted(self, payloads):
        """Device decode of every segment straight into the k-way merge-path
        merge (tzs_sorter_add_ifile_segment): no host parse, no re-sort.
        Returns the flushed sorter."""
        s = _engine.Sorter(self._conf())
        try:
            for payload, with_header in payloads:
                dev = _engine.upload_bytes(payload)
                try:
                    # partition -1: hash % 1 == 0, no explicit-partition path
                    s.add_ifile_segment(dev, len(payload), with_header=with_header,
                                        verify_crc=with_header, partition=-1)
                finally:
                    _engine.free_device(dev)
            s.flush()
            return s
        except BaseException:
            s.close()
            raise

    def _merge_resort(self, payloads):
        """Segments that are not sorted under this merge's key order (the
        engine's TezBytes order for variable-length keys depends on the
        partition count of the sorter that wrote them): decode on the device
        and let a fresh sorter re-sort the union.  Returns the flushed
        sorter."""
        s = _engine.Sorter(self._conf())
        try:
            for payload, with_header in payloads:
                dev = _engine.upload_bytes(payload)
                try:
                    d, off, kl, n = _engine.ifile_decode(
                        dev, len(payload), with_header=with_header,
                        verify_crc=with_header)
                finally:
                    _engine.free_device(dev)
                if n:
                    try:
                        s.write_batch_device(d, off, kl, None, n)
                    finally:
                        _engine.free_device(d, off, kl)
            s.flush()
            return s
        except BaseException:
            s.close()
            raise

    def start(self):
        """Merge the segments through the engine: each fetched segment is
        uploaded, decoded on the device and admitted as a sorted segment;
        flush runs the merge-path merge.  The key groups
        of the merged records are then built on the device and copied to the
        host as five arrays; the merged stream is not parsed.
        One partition in, one partition out."""
        self.close()
        payloads = [self._device_payload(seg) for seg in self._segments]
        try:
            s = self._merge_sorted(payloads)
        except _engine.EngineError as e:
            if e.rc != -22 or "not sorted" not in str(e):
                raise
            s = self._merge_resort(payloads)
        self._sorter = s
        g = s.grouped(0)
        try:
            self._grouped = GroupedKV(*g.to_host(), text_keys=self._text_keys)
        finally:
            g.free()
        return self

    def get_grouped(self):
        """The key groups of the merged input as a GroupedKV."""
        return self._grouped

    def get_reader(self):
        """KeyValuesReader: iterate (key_content, values list) groups."""
        return list(self.get_grouped())

    def get_reader_host(self):
        """The same groups from the merged IFile stream, downloaded here and
        parsed on the host: the yardstick for get_reader()."""
        data, index = self._sorter.output()
        st, raw, cl = index[0]
        merged = ifile.read_stream(data[st: st + cl]) if cl else []
        deser_k = ifile.deserialize_text if self._text_keys \
            else ifile.deserialize_bytes_writable
        groups = []
        prev_key = None
        for k, v, same in merged:
            if not same and (prev_key is None or k != prev_key):
                groups.append((deser_k(k), []))
            groups[-1][1].append(v)
            prev_key = k
        return groups

    def close(self):
        """Release the sorter kept for get_reader_host()."""
        if self._sorter is not None:
            self._sorter.close()
            self._sorter = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
