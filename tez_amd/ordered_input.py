"""OrderedGroupedKVInput — the reduce-side plugin surface
(input/OrderedGroupedKVInput.java:101-318) over the HIP engine.

Segments for THIS input's partition are added from producer outputs (the
local DISK_DIRECT path, FetcherOrderedGrouped.java:193-205, or the xGMI
exchange); start() runs the merge (Shuffle.run -> MergeManager.finalMerge
equivalents); get_reader() yields (key_content, [value_content...]) groups
with ValuesIterator semantics (ValuesIterator.java:177-199: same group iff
the merge reported SAME_KEY or the comparator says equal).
"""
import zlib

from . import _engine, ifile


class OrderedGroupedKVInput:
    def __init__(self, partition, props=None):
        self.partition = partition
        self.props = dict(props or {})
        self._segments = []
        self._merged = None
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
        merge (tzs_sorter_add_ifile_segment): no host parse, no re-sort."""
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
            return s.output()
        finally:
            s.close()

    def _merge_resort(self, payloads):
        """Segments that are not sorted under this merge's key order (the
        engine's TezBytes order for variable-length keys depends on the
        partition count of the sorter that wrote them): decode on the device
        and let a fresh sorter re-sort the union."""
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
            return s.output()
        finally:
            s.close()

    def start(self):
        """Merge the segments through the engine: each fetched segment is
        uploaded, decoded on the device and admitted as a sorted segment;
        flush runs the merge-path merge.  One partition
        in, one partition out."""
        payloads = [self._device_payload(seg) for seg in self._segments]
        try:
            data, index = self._merge_sorted(payloads)
        except _engine.EngineError as e:
            if e.rc != -22 or "not sorted" not in str(e):
                raise
            data, index = self._merge_resort(payloads)
        st, raw, cl = index[0]
        self._merged = ifile.read_stream(data[st: st + cl]) if cl else []
        return self

    def get_reader(self):
        """KeyValuesReader: iterate (key_content, values list) groups."""
        deser_k = ifile.deserialize_text if self._text_keys \
            else ifile.deserialize_bytes_writable
        groups = []
        prev_key = None
        for k, v, same in self._merged:
            if not same and (prev_key is None or k != prev_key):
                groups.append((deser_k(k), []))
            groups[-1][1].append(v)
            prev_key = k
        return groups
