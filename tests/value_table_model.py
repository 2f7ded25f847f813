"""A sequential model of the value table (NxgValueTable, include/nxg_codec.h).

State: slot -> value tree (the forms of tests/test_publish_values_cpu.py: ("sc", tag, fixed, aux),
("txt", tag, bytes), ("dec", bytes16), ("arr", [v..]), ("map", [(k, v)..]), ("err", v)), the four
counters, and the arrays exactly as the device must hold them: rows, the heap and the child
columns, appended to in slot order, each value written as `Layout` writes it (a container's
elements contiguous, blocks in depth-first preorder, payload bytes in visit order, no padding).

apply / rebuild / set_unsubscribed follow the header's semantics with every refusal: a refused
call raises before anything changes (Refused names the lowest slot and its cause; Capacity carries
the exact needs and the live totals the table would have).
"""
import numpy as np

MAX_DEPTH = 32  # NXG_MAX_DEPTH
TAG_UNSUBSCRIBED = 0x40
NULL = ("sc", 16, 0, 0)
UNSUBSCRIBED = ("sc", TAG_UNSUBSCRIBED, 0, 0)
# causes, as nxg_internal.h numbers them
ROW, TAG, HEAP, KIDS, NOKIDS, DEPTH, NOT_F64, SLOT = 1, 2, 3, 4, 5, 6, 7, 8
CAUSE_TEXT = {ROW: "src_row names a row", TAG: "a tag outside", HEAP: "a payload outside",
              KIDS: "a child range outside", NOKIDS: "a container without child columns",
              DEPTH: "nested deeper", NOT_F64: "NXG_NOT_F64", SLOT: "a slot at or past"}


OLD_SUFFIX = " (the value the table holds)"


class Refused(Exception):
    """old: the value refused is the one the table holds at `slot` (the replaced value of an
    apply, a value a rebuild carries over, the value set_unsubscribed drops)."""

    def __init__(self, slot, cause, old=False):
        super().__init__(f"slot {slot}: cause {cause}{OLD_SUFFIX if old else ''}")
        self.slot, self.cause, self.old = slot, cause, old


class Capacity(Exception):
    def __init__(self, need_bytes, need_children, live_bytes, live_children):
        super().__init__(f"need {need_bytes} bytes, {need_children} children")
        self.need_bytes, self.need_children = need_bytes, need_children
        self.live_bytes, self.live_children = live_bytes, live_children


class _Cause(Exception):
    def __init__(self, cause):
        self.cause = cause


class Source:
    """Values in columns: rows (tag None: all F64, aux None: 0), children (ctag None: no child
    columns), heap bytes, with the bounds the sizing pass checks against."""

    def __init__(self, tag, fixed, aux, ctag=None, cfixed=None, caux=None, heap=b"", n_rows=None,
                 n_children=None, heap_len=None):
        self.tag, self.fixed, self.aux = tag, fixed, aux
        self.ctag, self.cfixed, self.caux = ctag, cfixed, caux
        self.heap = bytes(heap)
        self.n_rows = len(fixed) if n_rows is None else n_rows
        self.n_children = (0 if ctag is None else len(ctag)) if n_children is None else n_children
        if self.n_children == 0:
            self.ctag = None
        self.heap_len = len(self.heap) if heap_len is None else heap_len

    def slot(self, child, i):
        if child:
            return int(self.ctag[i]), int(self.cfixed[i]), int(self.caux[i])
        return (9 if self.tag is None else int(self.tag[i]), int(self.fixed[i]),
                0 if self.aux is None else int(self.aux[i]))


def read_value(S, child, i, level=0):
    """The tree at (row | child slot) i, checked in walk order as the sizing pass checks it."""
    t, f, a = S.slot(child, i)
    if t > 27 and t != TAG_UNSUBSCRIBED:
        raise _Cause(TAG)
    if t in (12, 13, 18, 20, 27):
        n = 16 if t == 20 else a
        if f > S.heap_len or n > S.heap_len - f:
            raise _Cause(HEAP)
        b = S.heap[f:f + n]
        return ("dec", b) if t == 20 else ("txt", t, b)
    if t in (19, 21, 22):
        n = a if t == 19 else 2 * a if t == 21 else 1
        kids = []
        if n:
            if S.ctag is None:
                raise _Cause(NOKIDS)
            if f > S.n_children or n > S.n_children - f:
                raise _Cause(KIDS)
            if level >= MAX_DEPTH:  # its elements would sit past NXG_MAX_DEPTH
                raise _Cause(DEPTH)
            kids = [read_value(S, True, f + k, level + 1) for k in range(n)]
        if t == 19:
            return ("arr", kids)
        if t == 21:
            return ("map", [(kids[2 * k], kids[2 * k + 1]) for k in range(a)])
        return ("err", kids[0])
    return ("sc", t, f, a)


def elems(v):
    k = v[0]
    return v[1] if k == "arr" else [x for kv in v[1] for x in kv] if k == "map" else [v[1]]


def sizes(v):
    """(heap bytes, child slots, non-empty heap-borne leaves) of a tree."""
    k = v[0]
    if k == "sc":
        return 0, 0, 0
    if k == "txt":
        return len(v[2]), 0, 1 if v[2] else 0
    if k == "dec":
        return 16, 0, 1
    e = elems(v)
    b, c, l = 0, len(e), 0
    for x in e:
        sb, sc, sl = sizes(x)
        b, c, l = b + sb, c + sc, l + sl
    return b, c, l


def walk_branch(v):
    """Which walk a top-level value takes: 'scalar', 'leaf', 'flat' (registers), 'stack'."""
    if v[0] == "sc":
        return "scalar"
    if v[0] in ("txt", "dec"):
        return "leaf"
    return "stack" if any(x[0] in ("arr", "map", "err") for x in elems(v)) else "flat"


class Model:
    def __init__(self, n_slots, cap_bytes=0, cap_children=0, f64=False):
        self.n_slots, self.f64 = n_slots, f64
        self.cap_bytes = 0 if f64 else cap_bytes
        self.cap_children = 0 if f64 else cap_children
        self.init()

    # ---- the arrays ----------------------------------------------------------------------------
    def init(self):
        n = self.n_slots
        self.vals = [("sc", 9, 0, 0) if self.f64 else NULL] * n
        self.tag = np.full(n, 16, np.uint8)
        self.fixed = np.zeros(n, np.uint64)
        self.aux = np.zeros(n, np.uint32)
        self.heap = bytearray()
        self.ctag, self.cfixed, self.caux = [], [], []
        self.heap_live = self.child_live = 0
        return self

    heap_used = property(lambda self: len(self.heap))
    child_used = property(lambda self: len(self.ctag))

    def counters(self):
        return (self.heap_used, self.heap_live, self.child_used, self.child_live)

    def _emit(self, v):
        k = v[0]
        if k == "sc":
            return v[1], v[2], v[3]
        if k in ("txt", "dec"):
            t, b = (v[1], v[2]) if k == "txt" else (20, v[1])
            off = len(self.heap)
            self.heap += b
            return t, off, len(b)
        e = elems(v)
        base = len(self.ctag)
        self.ctag.extend([0] * len(e))
        self.cfixed.extend([0] * len(e))
        self.caux.extend([0] * len(e))
        for i, x in enumerate(e):
            self.ctag[base + i], self.cfixed[base + i], self.caux[base + i] = self._emit(x)
        return {"arr": 19, "map": 21, "err": 22}[k], base, len(v[1]) if k != "err" else 1

    def _store(self, s, v):
        self.vals[s] = v
        self.tag[s], self.fixed[s], self.aux[s] = self._emit(v)

    def arrays(self):
        return dict(tag=None if self.f64 else self.tag, fixed=self.fixed,
                    aux=None if self.f64 else self.aux,
                    heap=np.frombuffer(bytes(self.heap), np.uint8),
                    ctag=np.array(self.ctag, np.uint8), cfixed=np.array(self.cfixed, np.uint64),
                    caux=np.array(self.caux, np.uint32))

    # ---- the calls -----------------------------------------------------------------------------
    def _new(self, batch, src_row, s):
        """The tree slot s takes from the batch; raises Refused."""
        r = int(src_row[s]) - 1
        if r >= batch.n_rows:
            raise Refused(s, ROW)
        if self.f64 and batch.slot(False, r)[0] != 9:
            raise Refused(s, NOT_F64)
        try:
            return read_value(batch, False, r)
        except _Cause as c:
            raise Refused(s, c.cause)

    def _held(self):
        """The table's own arrays as a source: what it has written so far bounds every range.
        The values are read out of the arrays, not remembered: arrays a caller edited (or built
        itself) are validated like any input."""
        return Source(self.tag, self.fixed, self.aux, self.ctag, self.cfixed, self.caux,
                      bytes(self.heap), n_children=len(self.ctag))

    @staticmethod
    def _old(held, s):
        try:
            return read_value(held, False, s)
        except _Cause as c:
            raise Refused(s, c.cause, old=True)

    @staticmethod
    def _selection(batch, src_row, n_sel):
        if batch is None or src_row is None:
            return []
        return np.flatnonzero(np.asarray(src_row[:n_sel])).tolist()

    def apply(self, batch, src_row):
        """Returns the NxgValueApply dict."""
        slots = self._selection(batch, src_row, self.n_slots)
        if self.f64:
            sel = [(s, self._new(batch, src_row, s)) for s in slots]
            for s, v in sel:
                self.vals[s] = v
                self.fixed[s] = v[2]
            return dict(n_applied=len(sel), need_bytes=0, need_children=0, live_bytes=0,
                        live_children=0)
        held = self._held()
        sel = []
        nb = nc = ob = oc = 0
        for s in slots:  # ascending: the lowest refused slot, its new value before its old one
            v = self._new(batch, src_row, s)
            sel.append((s, v))
            b, c, _ = sizes(v)
            nb, nc = nb + b, nc + c
            b, c, _ = sizes(self._old(held, s))
            ob, oc = ob + b, oc + c
        live_b, live_c = self.heap_live - ob + nb, self.child_live - oc + nc
        if self.heap_used + nb > self.cap_bytes or self.child_used + nc > self.cap_children:
            raise Capacity(nb, nc, live_b, live_c)
        for s, v in sel:
            self._store(s, v)
        self.heap_live, self.child_live = live_b, live_c
        return dict(n_applied=len(sel), need_bytes=nb, need_children=nc, live_bytes=live_b,
                    live_children=live_c)

    def rebuild(self, n_slots, cap_bytes=0, cap_children=0, batch=None, src_row=None):
        """The table a rebuild into arrays of these capacities leaves (self is unchanged)."""
        assert n_slots >= self.n_slots
        chosen = set(self._selection(batch, src_row, self.n_slots))
        d = Model(n_slots, cap_bytes, cap_children, self.f64)
        held = None if self.f64 else self._held()
        sel, vals = {}, []
        for s in range(self.n_slots):  # a value carried over is walked, and validated, too
            if s in chosen:
                sel[s] = self._new(batch, src_row, s)
                vals.append(sel[s])
            else:
                vals.append(self.vals[s] if self.f64 else self._old(held, s))
        vals += [d.vals[0]] * (n_slots - self.n_slots)
        if self.f64:
            for s, v in enumerate(vals):
                d.vals[s] = v
                d.fixed[s] = v[2]
            return d, dict(n_applied=len(sel), need_bytes=0, need_children=0, live_bytes=0,
                           live_children=0)
        nb = sum(sizes(v)[0] for v in vals)
        nc = sum(sizes(v)[1] for v in vals)
        if nb > d.cap_bytes or nc > d.cap_children:
            raise Capacity(nb, nc, nb, nc)
        for s, v in enumerate(vals):
            d._store(s, v)
        d.heap_live, d.child_live = nb, nc
        return d, dict(n_applied=len(sel), need_bytes=nb, need_children=nc, live_bytes=nb,
                       live_children=nc)

    def set_unsubscribed(self, slots):
        bad = [int(s) for s in slots if int(s) >= self.n_slots]
        named = sorted(set(int(x) for x in slots) - set(bad))
        held = self._held()
        old = [self._old(held, s) for s in named]  # ascending: below any slot past the table
        if bad:
            raise Refused(min(bad), SLOT)
        for s, o in zip(named, old):
            b, c, _ = sizes(o)
            self.heap_live -= b
            self.child_live -= c
            self._store(s, UNSUBSCRIBED)


def table_trees(arr, heap_used, child_used):
    """The trees a table's arrays (host copies) hold, read back through the same checks."""
    S = Source(arr["tag"], arr["fixed"], arr["aux"], arr["ctag"], arr["cfixed"], arr["caux"],
               bytes(arr["heap"][:heap_used]) if arr["heap"] is not None else b"",
               n_children=child_used)
    return [read_value(S, False, s) for s in range(len(arr["fixed"]))]
