"""What the oneshot calls must produce (include/nxg_codec.h) -- TEST INFRASTRUCTURE, restated twice
without shared code, plus a port of the reply's decoder.

do_oneshot (netidx-archive/src/recorder/oneshot.rs:100-157) answers with OneshotReplyShard {
pathmap, image, deltas } inside OneshotReply(Vec<..>) (recorder_client.rs:29-37), both
#[derive(Pack)] and therefore length-wrapped (netidx-derive/src/lib.rs:113,137; pack.rs:522-525).

  restatement 1  a literal port of oneshot.rs:111-120 and 134-150 over Python objects (dicts and
                 lists of (Id, Event)), packed by line-by-line ports of the Pack impls: HashMap
                 (pack.rs:1107-1124, iterated in ascending Id order: a HashMap has none), VecDeque
                 (pack.rs:1057-1074), the tuple (pack.rs:1416-1424), DateTime<Utc> (pack.rs:
                 1555-1567), Vec<BatchItem> (pack.rs:941-952), Id (logfile/mod.rs:154-166), Path
                 (path.rs:61-68 over ArcStr, pack.rs:444-455). An Event is carried as its packed
                 bytes, written by tests/golden/make_golden.py's encoders (record_model.RowValues).
  restatement 2  numpy column-wise lengths and offsets; each record's batch bytes come from the
                 oracle's archive-batch encoder (oracle/nx_oracle.c through tests/nxo.py) over the
                 kept rows, through record_model.records_oracle.
  the decoder    OneshotReply::decode: len_wrapped_decode (pack.rs:537-556), HashMap / VecDeque /
                 Vec decode with check_sz! (pack.rs:919-939), DateTime decode, Event::decode
                 (logfile/mod.rs:188-205 over Value::decode's layout).
"""
import struct

import numpy as np

import record_model as rm
from record_model import NO_SLOT, RowValues

MAX_VEC = 2 * 1024 * 1024 * 1024
PATHMAP_ENTRY = 12        # size_of::<Id>() + size_of::<Path>() (an ArcStr is one pointer)
BATCH_ITEM = 24           # size_of::<BatchItem>()
MAX_ELEMS = MAX_VEC // 64  # n_deltas and n_shards (the elements' sizes involve GPooled: unpinned)
U64 = (1 << 64) - 1


class TooBig(Exception):
    pass


class BufferShort(Exception):
    pass


class InvalidFormat(Exception):
    pass


# ---- pack.rs scalars ----------------------------------------------------------------------------
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


# ---- the cases ------------------------------------------------------------------------------------
class Paths:
    """A shard's path index in Id order and the host's filter: paths[a] (bytes; empty: Id a has
    no path), keep[a]."""

    def __init__(self, paths, keep):
        self.paths = [bytes(p) for p in paths]
        self.keep = np.asarray(keep, np.uint8)
        assert len(self.paths) == len(self.keep)

    n_ids = property(lambda self: len(self.paths))

    def path_off(self):
        off = np.zeros(self.n_ids + 1, np.uint64)
        off[1:] = np.cumsum([len(p) for p in self.paths])
        return off

    def path_bytes(self):
        return np.frombuffer(b"".join(self.paths), np.uint8)


class Window:
    """One decoded window: the columns (a value_table_model.Source), the id column, the records
    as (row_off, n_rows), their timestamps, and the filter set: n_ids and the selected Ids."""

    def __init__(self, src, ids, recs, secs, nanos, n_ids, selected):
        self.src = src
        self.ids = np.asarray(ids, np.uint64)
        self.recs = [(int(a), int(b)) for a, b in recs]
        self.secs = [int(s) for s in secs]
        self.nanos = [int(x) for x in nanos]
        self.n_ids = int(n_ids)
        self.selected = frozenset(int(a) for a in selected)
        assert len(self.ids) == src.n_rows and len(self.recs) == len(self.secs) == len(self.nanos)
        assert all(a < self.n_ids for a in self.selected)

    n_recs = property(lambda self: len(self.recs))

    def is_sel(self, a):
        return a < self.n_ids and a in self.selected

    def rows(self):
        """The window rows of all records, in order, and the records' offsets into that list."""
        rows = np.concatenate([np.arange(a, a + n, dtype=np.int64) for a, n in self.recs] +
                              [np.zeros(0, np.int64)])
        off = np.zeros(self.n_recs + 1, np.int64)
        off[1:] = np.cumsum([n for _, n in self.recs])
        return rows, off

    def as_record_case(self):
        """The same filter as an nxg_record_entries call: entry = row, channel = record, SubIds
        numbering the distinct Ids, the table holding the Id itself or NO_SLOT."""
        rows, off = self.rows()
        ids = self.ids[rows]
        uniq, sub = np.unique(ids, return_inverse=True)
        arch = np.array([int(a) if self.is_sel(int(a)) else NO_SLOT for a in uniq], np.uint32)
        return rm.Case(self.src, sub.astype(np.uint64), rows.astype(np.uint64), off, arch)


# ---- restatement 1: the reference's objects and its Pack impls --------------------------------------
def do_oneshot_pathmap(paths):
    """oneshot.rs:111-120: (filterset, pathmap) from iter_pathmap() and filter.is_match."""
    filterset, pathmap = set(), {}
    for a, path in enumerate(paths.paths):
        if not path:          # (the index has no entry for this Id)
            continue
        if paths.keep[a]:     # args.filter.is_match(path)
            filterset.add(a)
            pathmap[a] = path
    return filterset, pathmap


def read_deltas(win):
    """What read_deltas hands to oneshot.rs:141: [(timestamp, [BatchItem(id, event)])]."""
    vals = RowValues(win.src)
    return [((win.secs[i], win.nanos[i]),
             [(int(win.ids[r]), vals.event(r)) for r in range(a, a + n)])
            for i, (a, n) in enumerate(win.recs)]


def do_oneshot_deltas(pathmap, batches):
    """oneshot.rs:146-150: retain_mut over the window's batches."""
    out = []
    for ts, batch in batches:
        batch = [(i, ev) for i, ev in batch if i in pathmap]   # batch.retain(contains_key)
        if batch:                                              # !batch.is_empty()
            out.append((ts, batch))
    return out


def pack_id(i):  # logfile/mod.rs:154-166
    return encode_varint(i)


def pack_path(p):  # path.rs:61-68 -> ArcStr, pack.rs:451-455
    return encode_varint(len(p)) + p


def pack_hashmap(m, entry_size, pack_v):  # pack.rs:1113-1124, ascending keys
    if len(m) * entry_size > MAX_VEC:
        raise TooBig()
    out = [encode_varint(len(m))]
    for k in sorted(m):
        out.append(pack_id(k))
        out.append(pack_v(m[k]))
    return b"".join(out)


def pack_datetime(ts):  # pack.rs:1555-1567: put_i64(timestamp), put_u32(subsec nanos)
    return struct.pack(">qI", ts[0], ts[1])


def pack_batch(batch):  # pack.rs:941-952 over BatchItem (logfile/mod.rs:188-205)
    if len(batch) * BATCH_ITEM > MAX_VEC:
        raise TooBig()
    return encode_varint(len(batch)) + b"".join(pack_id(i) + ev for i, ev in batch)


def pack_delta(d):  # the tuple, pack.rs:1416-1424
    return pack_datetime(d[0]) + pack_batch(d[1])


def pack_deltas(deltas):  # VecDeque, pack.rs:1064-1074
    if len(deltas) > MAX_ELEMS:
        raise TooBig()
    return encode_varint(len(deltas)) + b"".join(pack_delta(d) for d in deltas)


def pack_shard(pathmap, image, deltas):  # derive(Pack), named fields in order
    inner = (pack_hashmap(pathmap, PATHMAP_ENTRY, pack_path) +
             pack_hashmap(image, 4 + 8, lambda ev: ev) + pack_deltas(deltas))
    return encode_varint(len_wrapped_len(len(inner))) + inner


def pack_reply(shards):  # derive(Pack) over the one Vec field
    if len(shards) > MAX_ELEMS:
        raise TooBig()
    inner = encode_varint(len(shards)) + b"".join(shards)
    return encode_varint(len_wrapped_len(len(inner))) + inner


def pathmap_python(paths):
    """(section bytes, sel) by restatement 1."""
    filterset, pathmap = do_oneshot_pathmap(paths)
    sel = np.zeros(paths.n_ids, np.uint8)
    sel[sorted(filterset)] = 1
    return pack_hashmap(pathmap, PATHMAP_ENTRY, pack_path), sel


def deltas_python(win):
    """[element bytes per record] ('' for a record dropped whole) by restatement 1."""
    pathmap = {a: b"" for a in win.selected}
    out = []
    for ts, batch in read_deltas(win):
        kept = do_oneshot_deltas(pathmap, [(ts, batch)])
        out.append(pack_delta(kept[0]) if kept else b"")
    return out


# ---- restatement 2: columns and the oracle ------------------------------------------------------------
def _vl(v):
    v = np.asarray(v, np.uint64)
    return 1 + sum((v >= np.uint64(1 << s)).astype(np.int64) for s in (7, 14, 21, 28, 35, 42, 49, 56, 63))


def pathmap_numpy(paths):
    """(section bytes, sel, n_sel) column-wise."""
    off = paths.path_off().astype(np.int64)
    plen = np.diff(off)
    sel = ((paths.keep != 0) & (plen > 0)).astype(np.uint8)
    ids = np.flatnonzero(sel)
    lens = _vl(ids) + _vl(plen[ids]) + plen[ids]
    head = varint_len(len(ids))
    at = head + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out = np.zeros(int(at[-1]), np.uint8)
    out[:head] = np.frombuffer(encode_varint(len(ids)), np.uint8)
    blob = paths.path_bytes()
    for j, a in enumerate(ids):
        h = encode_varint(int(a)) + encode_varint(int(plen[a]))
        p = int(at[j])
        out[p:p + len(h)] = np.frombuffer(h, np.uint8)
        out[p + len(h):int(at[j + 1])] = blob[off[a]:off[a + 1]]
    return out.tobytes(), sel, len(ids)


def deltas_oracle(win):
    """[element bytes per record]: the timestamp in front of the oracle's archive batch of the
    kept rows."""
    case = win.as_record_case()
    recs = rm.records_oracle(case)
    return [struct.pack(">qI", win.secs[i], win.nanos[i]) + r if r else b""
            for i, r in enumerate(recs)]


def expected_deltas(win, elements=None):
    """(blob, rec_off, rec_items, n_items, n_dropped, n_kept_recs) of a call that succeeds."""
    el = deltas_oracle(win) if elements is None else elements
    rows, off = win.rows()
    kept = np.array([win.is_sel(int(a)) for a in win.ids[rows]], bool)
    items = np.array([int(kept[off[i]:off[i + 1]].sum()) for i in range(win.n_recs)], np.uint64)
    rec_off = np.zeros(win.n_recs + 1, np.uint64)
    rec_off[1:] = np.cumsum([len(e) for e in el])
    return (b"".join(el), rec_off, items, int(items.sum()), len(rows) - int(items.sum()),
            int((items != 0).sum()))


def deltas_refusal(win):
    """None, ("row", r, cause) for the lowest kept window row that is refused, or ("vec", i). An
    item of 2^32 bytes or more is a size guard too (the bound nxg_encode_archive_batch puts on an
    item): only a String / Bytes / Error(String) / Abstract row can reach it, by its length alone."""
    case = win.as_record_case()
    r = rm.refusal(case)
    kept, _ = case.keep()
    S = win.src
    long_item = None
    for e in np.flatnonzero(kept):
        row = int(case.ent_row[e])
        t, a = int(S.tag[row]), int(S.aux[row])
        body = a + varint_len(a) if t in (12, 13, 18) else len_wrapped_len(a) if t == 27 else 0
        if varint_len(int(win.ids[row])) + 1 + body > 0xFFFFFFFF:
            long_item = (int(e), row)
            break
    if long_item and (r is None or r[0] != "entry" or long_item[0] < r[1]):
        return ("row", long_item[1], rm.BIG)
    if r is None:
        return None
    if r[0] == "entry":
        return ("row", int(case.ent_row[r[1]]), r[2])
    assert r[0] == "vec"
    return r


# ---- the framing ---------------------------------------------------------------------------------------
def shard_layout(pathmap_len, image_len, deltas_len, n_deltas):
    """What nxg_oneshot_shard_layout must answer, as a dict."""
    if n_deltas > MAX_ELEMS:
        raise TooBig()
    count = encode_varint(n_deltas)
    inner = pathmap_len + image_len + len(count) + deltas_len
    head = encode_varint(len_wrapped_len(inner))
    po = len(head)
    return dict(len_head=head, count_head=count, pathmap_off=po, image_off=po + pathmap_len,
                count_off=po + pathmap_len + image_len,
                deltas_off=po + pathmap_len + image_len + len(count),
                shard_len=po + inner)


def reply_head(shard_lens):
    if len(shard_lens) > MAX_ELEMS:
        raise TooBig()
    inner = varint_len(len(shard_lens)) + sum(shard_lens)
    head = encode_varint(len_wrapped_len(inner))
    return head + encode_varint(len(shard_lens)), len(head) + inner


# ---- the decoder -----------------------------------------------------------------------------------------
class Buf:
    """bytes::Buf over a slice with Take's limit."""

    def __init__(self, b, pos=0, end=None):
        self.b, self.pos, self.end = b, pos, len(b) if end is None else end

    def remaining(self):
        return self.end - self.pos

    def get(self, n):
        if n > self.remaining():
            raise BufferShort()
        out = self.b[self.pos:self.pos + n]
        self.pos += n
        return bytes(out)


def decode_varint(buf):  # pack.rs:504-520
    value = 0
    for i in range(10):
        if buf.remaining() < 1:
            raise BufferShort()
        byte = buf.get(1)[0]
        value |= ((byte & 0x7F) << (i * 7)) & U64
        if byte <= 0x7F:
            return value
    raise InvalidFormat()


def check_sz(elts, remaining, size):  # pack.rs:919-939
    if elts * size > MAX_VEC or elts > remaining:
        raise TooBig()


def decode_value(buf, depth=0):
    """The extent of one Value (netidx-value/src/lib.rs Value::decode's layout): its bytes."""
    start = buf.pos
    t = buf.get(1)[0]
    if t in (0, 2, 8):
        buf.get(4)
    elif t in (1, 3, 5, 7):
        decode_varint(buf)
    elif t in (4, 6, 9):
        buf.get(8)
    elif t in (10, 11):
        buf.get(12)
    elif t in (12, 13, 18):
        buf.get(decode_varint(buf))
    elif t in (14, 15, 16):
        pass
    elif t == 19:
        for _ in range(decode_varint(buf)):
            decode_value(buf, depth + 1)
    elif t == 20:
        buf.get(16)
    elif t == 21:
        for _ in range(2 * decode_varint(buf)):
            decode_value(buf, depth + 1)
    elif t == 22:
        decode_value(buf, depth + 1)
    elif t in (23, 24):
        buf.get(1)
    elif t in (25, 26):
        buf.get(2)
    elif t == 27:
        ln = decode_varint(buf)
        buf.get(ln - varint_len(ln))
    else:
        raise InvalidFormat()
    return bytes(buf.b[start:buf.pos])


def decode_event(buf):  # logfile/mod.rs:188-205: 0x40 is Unsubscribed, else the Value
    if buf.remaining() < 1:
        raise BufferShort()
    if buf.b[buf.pos] == 0x40:
        return buf.get(1)
    return decode_value(buf)


def len_wrapped_decode(buf):  # pack.rs:537-556: the limited view, and what to skip behind it
    ln = decode_varint(buf)
    if ln < 1:
        raise BufferShort()
    n = ln - varint_len(ln)
    if n > buf.remaining():
        raise BufferShort()
    return Buf(buf.b, buf.pos, buf.pos + n)


def decode_hashmap(buf, size, decode_v):  # pack.rs:1126-1136
    elts = decode_varint(buf)
    check_sz(elts, buf.remaining(), size)
    out = {}
    for _ in range(elts):
        k = decode_varint(buf)
        out[k] = decode_v(buf)
    return out


def decode_path(buf):
    ln = decode_varint(buf)
    if ln > buf.remaining():
        raise TooBig()
    return buf.get(ln)


def decode_shard(buf):
    lim = len_wrapped_decode(buf)
    pathmap = decode_hashmap(lim, PATHMAP_ENTRY, decode_path)
    image = decode_hashmap(lim, 12, decode_event)
    elts = decode_varint(lim)
    check_sz(elts, lim.remaining(), 64)
    deltas = []
    for _ in range(elts):
        secs, nanos = struct.unpack(">qI", lim.get(12))
        n = decode_varint(lim)
        check_sz(n, lim.remaining(), BATCH_ITEM)
        batch = []
        for _ in range(n):
            i = decode_varint(lim)
            batch.append((i, decode_event(lim)))
        deltas.append(((secs, nanos), batch))
    if lim.remaining():
        raise InvalidFormat()
    buf.pos = lim.end
    return pathmap, image, deltas


def decode_reply(b):
    """OneshotReply::decode: [(pathmap, image, deltas) per shard]."""
    buf = Buf(b)
    lim = len_wrapped_decode(buf)
    elts = decode_varint(lim)
    check_sz(elts, lim.remaining(), 64)
    shards = [decode_shard(lim) for _ in range(elts)]
    if lim.remaining() or lim.end != len(b):
        raise InvalidFormat()
    return shards
