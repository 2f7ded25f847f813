"""What nxg_record_entries must produce (include/nxg_codec.h), built two ways that share no code.

The recorder's batch loop (netidx-archive/src/recorder/record.rs:307-347): per channel, every entry
(SubId, Event) is translated through by_subid, dropped when it has no archive Id, and the rest
become one archive batch, <Vec<BatchItem> as Pack>::encode (pack.rs:941-952); an empty batch
writes nothing (writer.rs:405).

  records_oracle   per channel: filter and translate in numpy, gather the kept rows into an
                   nxo.Decoded with id = arch_id (tag 0x40 for span entries), nxo.encode_archive
  records_python   a pure-Python item writer on varint_len / enc_varint / enc_value / archive of
                   tests/golden/make_golden.py, reading the value trees out of the columns

`refusal` states which false return a case gets and what its message names; `item_lens` the
per-entry lengths the kernels' plan (tests/record_cases.py) is computed from.
"""
import os
import sys

import numpy as np

import nxo
from value_table_model import Source, read_value

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden as mg  # noqa: E402

NO_SLOT = 0xFFFFFFFF
ENT_SPAN = 1 << 63
TAG_UNSUBSCRIBED = 0x40
MAX_DEPTH = 32
MAX_VEC = 2 * 1024 * 1024 * 1024
BATCH_ITEM_SIZE = 24
MAX_ITEMS = MAX_VEC // BATCH_ITEM_SIZE  # the most items a record may hold

# causes of a refused entry, and the words of the message that name them
ROW, TAG, BIG, KIDS, NOKIDS, DEPTH = 1, 2, 3, 4, 5, 6
CAUSE_TEXT = {ROW: "ent_row names a row at or past", TAG: "an unknown tag", BIG: "a size guard",
              KIDS: "a child range outside", NOKIDS: "a container with elements but no child",
              DEPTH: "nested deeper than NXG_MAX_DEPTH"}


class Case:
    """One call: the batch (a value_table_model.Source; tag None: F64 layout), the entry list and
    the recorder's table."""

    def __init__(self, src, ent_sub, ent_row, chan_off, arch):
        self.src = src
        self.ent_sub = np.asarray(ent_sub, np.uint64)
        self.ent_row = np.asarray(ent_row, np.uint64)
        self.chan_off = np.asarray(chan_off, np.uint64)
        self.arch = np.asarray(arch, np.uint32)
        assert len(self.ent_sub) == len(self.ent_row)

    n_entries = property(lambda self: len(self.ent_sub))
    n_chans = property(lambda self: len(self.chan_off) - 1)

    def f64_layout(self):
        """The same call on F64-layout columns (every row must be an F64)."""
        assert self.src.tag is not None and (self.src.tag == 9).all()
        return Case(Source(None, self.src.fixed, None), self.ent_sub, self.ent_row, self.chan_off,
                    self.arch)

    def keep(self):
        """(kept flag, archive Id) per entry; entries in front of chan_off[0] belong to no
        channel."""
        sub = self.ent_sub
        known = sub < len(self.arch)
        aid = np.full(len(sub), NO_SLOT, np.uint32)
        aid[known] = self.arch[sub[known].astype(np.int64)]
        kept = aid != NO_SLOT
        kept[: min(int(self.chan_off[0]), len(sub))] = False
        return kept, aid

    def is_span(self):
        return (self.ent_row & np.uint64(ENT_SPAN)) != 0


# ---- refusals -----------------------------------------------------------------------------------
def value_cause(S, row):
    """The first refusal in walk order of the value in row `row`, or 0."""
    def walk(child, i, level):
        t, f, a = S.slot(child, i)
        if level > MAX_DEPTH:
            return DEPTH
        if t in (19, 21, 22):
            if t != 22 and a * (16 if t == 19 else 32) > MAX_VEC:
                return BIG
            n = a if t == 19 else 2 * a if t == 21 else 1
            if n:
                if S.ctag is None:
                    return NOKIDS
                if f > S.n_children or n > S.n_children - f:
                    return KIDS
            for k in range(n):
                c = walk(True, f + k, level + 1)
                if c:
                    return c
            return 0
        return TAG if t > 27 or t == 17 else 0

    if not (S.tag is None) and int(S.tag[row]) == TAG_UNSUBSCRIBED:
        return 0
    return walk(False, row, 0)


def refusal(case):
    """None, or what the call refuses: ("chan", c), ("entry", e, cause) or ("vec", c), in the
    order the call reports them."""
    off, n = case.chan_off.astype(np.int64), case.n_entries
    for c in range(case.n_chans):
        if off[c + 1] < off[c] or (c == case.n_chans - 1 and off[c + 1] != n):
            return ("chan", c)
    if case.n_chans == 0 and off[0] != n:
        return ("chan", 0)
    kept, _ = case.keep()
    span = case.is_span()
    seen = {}
    for e in np.flatnonzero(kept & ~span):
        r = int(case.ent_row[e])
        if r not in seen:
            seen[r] = ROW if r >= case.src.n_rows else value_cause(case.src, r)
        if seen[r]:
            return ("entry", int(e), seen[r])
    for c in range(case.n_chans):
        if int(kept[off[c]:off[c + 1]].sum()) > MAX_ITEMS:
            return ("vec", c)
    return None


# ---- the records, by the oracle -------------------------------------------------------------------
def records_oracle(case):
    """[record bytes per channel], by nxo.encode_archive over the gathered kept rows."""
    S = case.src
    kept, aid = case.keep()
    span = case.is_span()
    nk = S.n_children
    out = []
    for c in range(case.n_chans):
        lo, hi = int(case.chan_off[c]), int(case.chan_off[c + 1])
        idx = lo + np.flatnonzero(kept[lo:hi])
        if not len(idx):
            out.append(b"")
            continue
        sp = span[idx]
        rows = np.where(sp, 0, case.ent_row[idx]).astype(np.int64)
        d = nxo.Decoded(len(idx), max(nk, 1), 1)
        d.id[:] = aid[idx]
        d.tag[:] = np.where(sp, TAG_UNSUBSCRIBED, 9 if S.tag is None else S.tag[rows])
        d.fixed[:] = np.where(sp, 0, S.fixed[rows])
        d.aux[:] = 0 if S.aux is None else np.where(sp, 0, S.aux[rows])
        if nk:
            d.ctag[:nk], d.cfixed[:nk], d.caux[:nk] = S.ctag, S.cfixed, S.caux
        d.s.n_rows, d.s.n_children = len(idx), nk
        out.append(nxo.encode_archive(d, S.heap))
    return out


# ---- the records, in pure Python ------------------------------------------------------------------
def _signed(x, bits):
    x &= (1 << bits) - 1
    return x - (1 << bits) if x >> (bits - 1) else x


def golden_value(v):
    """A value tree (value_table_model) as make_golden's (tag, payload)."""
    k = v[0]
    if k == "sc":
        t, f, a = v[1], v[2], v[3]
        if t in (0, 1, 8):
            return (t, f & 0xFFFFFFFF)
        if t in (2, 3):
            return (t, _signed(f, 32))
        if t in (4, 5, 9):
            return (t, f)
        if t in (6, 7):
            return (t, _signed(f, 64))
        if t == 10:
            return (t, (_signed(f, 64), a))
        if t == 11:
            return (t, (f, a))
        if t in (14, 15, 16):
            return (t, None)
        if t in (23, 25):
            return (t, f & (0xFF if t == 23 else 0xFFFF))
        if t in (24, 26):
            return (t, _signed(f, 8 if t == 24 else 16))
        raise ValueError(t)
    if k == "txt":
        return (v[1], v[2])
    if k == "dec":
        return (20, v[1])
    if k == "arr":
        return (19, [golden_value(x) for x in v[1]])
    if k == "map":
        return (21, [(golden_value(a), golden_value(b)) for a, b in v[1]])
    return (22, golden_value(v[1]))


class RowValues:
    """Event bytes per batch row, encoded once per row."""

    def __init__(self, S):
        self.S = Source(S.tag, S.fixed, S.aux, S.ctag, S.cfixed, S.caux, S.heap,
                        heap_len=1 << 62)  # (this call bounds no payload by a heap length)
        self.memo = {}

    def event(self, row):
        b = self.memo.get(row)
        if b is None:
            if self.S.tag is not None and int(self.S.tag[row]) == TAG_UNSUBSCRIBED:
                b = bytes([mg.UNSUB])
            else:
                b = mg.enc_value(golden_value(read_value(self.S, False, row)))
            self.memo[row] = b
        return b


def records_python(case):
    """[record bytes per channel], items written by make_golden's encoders; each record is also
    what make_golden.archive writes for the channel's (Id, value) list."""
    kept, aid = case.keep()
    span = case.is_span()
    vals = RowValues(case.src)
    out = []
    for c in range(case.n_chans):
        lo, hi = int(case.chan_off[c]), int(case.chan_off[c + 1])
        items = []
        for e in range(lo, hi):
            if kept[e]:
                ev = bytes([mg.UNSUB]) if span[e] else vals.event(int(case.ent_row[e]))
                items.append(mg.enc_varint(int(aid[e])) + ev)
        out.append(mg.enc_varint(len(items)) + b"".join(items) if items else b"")
    return out


def item_lens(case):
    """Per entry: the bytes of its item, varint(Id) + Event (0: not kept)."""
    kept, aid = case.keep()
    span = case.is_span()
    vals = RowValues(case.src)
    n_rows = case.src.n_rows
    rows = np.where(span | ~kept, 0, case.ent_row).astype(np.int64)
    used = np.unique(rows[kept & ~span])
    vlen = np.zeros(max(n_rows, 1), np.int64)
    for r in used:
        vlen[r] = len(vals.event(int(r)))
    a = aid.astype(np.int64)
    idl = 1 + sum((a >= (1 << s)).astype(np.int64) for s in (7, 14, 21, 28))
    return np.where(kept, idl + np.where(span, 1, vlen[rows]), 0)


def expected(case, records=None):
    """(blob, rec_off, rec_items, n_dropped) of a call that succeeds."""
    rec = records_oracle(case) if records is None else records
    kept, _ = case.keep()
    off = case.chan_off.astype(np.int64)
    items = np.array([int(kept[off[c]:off[c + 1]].sum()) for c in range(case.n_chans)], np.uint64)
    rec_off = np.zeros(case.n_chans + 1, np.uint64)
    rec_off[1:] = np.cumsum([len(r) for r in rec])
    n_in = case.n_entries - min(int(off[0]), case.n_entries)
    return b"".join(rec), rec_off, items, n_in - int(kept.sum())


def f64_closed_form(n_items, arch_id):
    """n_bytes of one channel of n_items F64 items that all carry arch_id."""
    return mg.varint_len(n_items) + n_items * (mg.varint_len(arch_id) + 9) if n_items else 0
