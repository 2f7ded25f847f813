"""What nxg_archive_index_records and nxg_archive_scan_index must produce (include/nxg_codec.h) --
TEST INFRASTRUCTURE, written from the reference's lines, not from the kernels.

The writer (add_batch, netidx-archive/src/logfile/writer.rs:407-429, and #[derive(Pack)] struct
RecordIndex { index: Vec<Id> }, logfile/mod.rs:146-149) is written twice, sharing no code:
`indexes_python` is the HashSet loop with a list beside the set (first occurrence is the order the
library pins), `indexes_numpy` finds the first occurrences with np.unique and encodes the varints
column-wise. The scanner, `scan_index_at`, is a literal port of reader.rs:394-422 over a bytes
slice, with the two deviations the header documents.
"""
import numpy as np

NO_SLOT = 0xFFFFFFFF
NONE, MATCH, ERR_SHORT, ERR_FORMAT = 0, 1, 2, 3
MAX_VEC = 2 * 1024 * 1024 * 1024
U64 = (1 << 64) - 1


class Case:
    """key[p] over records [seg_off[c], seg_off[c+1]); table None (key holds Ids) or
    arch_id_of_sub."""

    def __init__(self, key, seg_off, table=None):
        self.key = np.ascontiguousarray(key, dtype=np.uint64)
        self.seg_off = np.ascontiguousarray(seg_off, dtype=np.uint64)
        self.table = None if table is None else np.ascontiguousarray(table, dtype=np.uint32)

    @property
    def n_keys(self):
        return len(self.key)

    @property
    def n_recs(self):
        return len(self.seg_off) - 1


# ---- the writer, the reference's loop ----------------------------------------------------------
def varint_len(v):  # pack.rs:472-474
    return (((63 - ((v | 1).bit_length() - 1)) ^ 63) * 9 + 73) >> 6


def encode_varint(v):  # pack.rs:476-486
    out = bytearray()
    for _ in range(10):
        if v < 0x80:
            out.append(v)
            break
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    return bytes(out)


def len_wrapped_len(n):  # pack.rs:522-525
    return n + varint_len(n + varint_len(n))


def record_index(ids):
    """<RecordIndex as Pack>::encode: the length-wrapped struct whose one field is Vec<Id>."""
    inner = encode_varint(len(ids)) + b"".join(encode_varint(i) for i in ids)
    return encode_varint(len_wrapped_len(len(inner))) + inner


def refusal(case):
    """None, ("seg", c) for the lowest record where seg_off decreases (or the last when it ends
    behind the keys), ("wide", p) for the lowest position of a record whose Id is >= 2^32, or
    ("vec", c)."""
    off = [int(x) for x in case.seg_off]
    for c in range(case.n_recs):
        if off[c + 1] < off[c]:
            return ("seg", c)
    if case.n_recs and off[-1] > case.n_keys:
        return ("seg", case.n_recs - 1)
    if case.table is None and case.n_recs:
        wide = np.flatnonzero(case.key[off[0]:off[-1]] > 0xFFFFFFFF)
        if len(wide):
            return ("wide", off[0] + int(wide[0]))
    return None


def kept_id(case, p):
    k = int(case.key[p])
    if case.table is None:
        return k
    if k >= len(case.table) or int(case.table[k]) == NO_SLOT:
        return None
    return int(case.table[k])


def indexes_python(case):
    """Per record: the bytes of its RecordIndex (b"" for a record that keeps nothing) and its Ids."""
    out = []
    for c in range(case.n_recs):
        seen, order = set(), []
        for p in range(int(case.seg_off[c]), int(case.seg_off[c + 1])):
            i = kept_id(case, p)
            if i is not None and i not in seen:
                seen.add(i)
                order.append(i)
        assert len(order) * 4 <= MAX_VEC
        out.append((record_index(order) if order else b"", order))
    return out


# ---- the writer, column-wise ----------------------------------------------------------------------
def _vl_np(v):
    v = v.astype(np.uint64)
    n = np.ones(len(v), np.int64)
    for s in range(7, 64, 7):
        n += v >= np.uint64(1 << s)
    return n


def _varints_np(v):
    """The concatenated varints of v as a uint8 array."""
    v = v.astype(np.uint64)
    w = _vl_np(v)
    start = np.concatenate([[0], np.cumsum(w)])
    out = np.zeros(int(start[-1]), np.uint8)
    for k in range(10):
        m = w > k
        if not m.any():
            break
        b = (v[m] >> np.uint64(7 * k)) & np.uint64(0x7F)
        b |= np.where(w[m] > k + 1, np.uint64(0x80), np.uint64(0))
        out[start[:-1][m] + k] = b.astype(np.uint8)
    return out


def indexes_numpy(case):
    """(blob, idx_off, idx_ids): all records' indexes back to back."""
    nr = case.n_recs
    off = case.seg_off.astype(np.int64)
    lo, hi = int(off[0]), int(off[-1])
    pos = np.arange(lo, hi, dtype=np.int64)
    rec = np.searchsorted(off[1:], pos, side="right")
    k = case.key[lo:hi]
    if case.table is None:
        ids, kept = k, np.ones(len(k), bool)
    else:
        known = k < np.uint64(len(case.table))
        ids = np.where(known, case.table[np.where(known, k, 0).astype(np.int64)] if len(case.table)
                       else 0, NO_SLOT).astype(np.uint64)
        kept = ids != NO_SLOT
    pair = (rec.astype(np.uint64) << np.uint64(32)) | (ids & np.uint64(0xFFFFFFFF))
    _, first = np.unique(pair[kept], return_index=True)
    first = np.sort(np.flatnonzero(kept)[first])  # positions (relative to lo) of first occurrences
    frec, fid = rec[first], ids[first]
    count = np.bincount(frec, minlength=nr).astype(np.int64)
    idb = np.bincount(frec, weights=_vl_np(fid), minlength=nr).astype(np.int64)
    has = count > 0
    inner = np.where(has, _vl_np(count) + idb, 0)
    L = inner + _vl_np(inner + _vl_np(inner))
    lead = np.where(has, _vl_np(L) + _vl_np(count), 0)
    size = np.where(has, lead + idb, 0)
    idx_off = np.concatenate([[0], np.cumsum(size)]).astype(np.uint64)
    blob = np.zeros(int(idx_off[-1]), np.uint8)
    # the leads
    for c in np.flatnonzero(has):
        h = np.concatenate([_varints_np(np.array([L[c]])), _varints_np(np.array([count[c]]))])
        blob[int(idx_off[c]):int(idx_off[c]) + len(h)] = h
    # the Ids: record c's start at idx_off[c] + lead[c], in first-occurrence order
    vb = _varints_np(fid)
    w = _vl_np(fid)
    src = np.concatenate([[0], np.cumsum(w)])[:-1]
    before = np.concatenate([[0], np.cumsum(idb)])[:-1]  # Id bytes of the records in front
    dst = src - before[frec] + idx_off[:-1].astype(np.int64)[frec] + lead[frec]
    for kk in range(5):
        m = w > kk
        blob[dst[m] + kk] = vb[src[m] + kk]
    return blob.tobytes(), idx_off, count.astype(np.uint64)


def expected(case):
    """(blob, idx_off, idx_ids) by the loop."""
    recs = indexes_python(case)
    off = np.concatenate([[0], np.cumsum([len(b) for b, _ in recs])]).astype(np.uint64)
    return (b"".join(b for b, _ in recs), off,
            np.array([len(o) for _, o in recs], np.uint64))


# ---- the scanner ------------------------------------------------------------------------------------
class BufferShort(Exception):
    code = ERR_SHORT


class InvalidFormat(Exception):
    code = ERR_FORMAT


def decode_varint(buf, pos):  # pack.rs:504-520 over the chunk buf[pos:]: (value, the position behind)
    value = 0
    for i in range(10):
        if pos + i >= len(buf):
            raise BufferShort()
        byte = buf[pos + i]
        value |= ((byte & 0x7F) << (i * 7)) & U64
        if byte <= 0x7F:
            return value, pos + i + 1
    raise InvalidFormat()


def scan_index_at(data, pos, end, keep):
    """reader.rs:413-421 from the RecordIndex on: data[pos:end] is the record from its index to
    its end; keep a uint8 array indexed by Id. Deviations: the slice ends at the record's end, and
    index_len == 0 (an underflow in the reference) is InvalidFormat."""
    buf = bytes(data[pos:end])
    try:
        index_len, p = decode_varint(buf, 0)
        if index_len == 0:
            raise InvalidFormat()
        buf = buf[p:p + index_len - varint_len(index_len)]  # Buf::take clips
        p = 0
        while p < len(buf):
            i, p = decode_varint(buf, p)
            i &= 0xFFFFFFFF  # Id(id as u32)
            if i < len(keep) and keep[i]:
                return MATCH
        return NONE
    except (BufferShort, InvalidFormat) as e:
        return e.code
