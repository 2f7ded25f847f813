"""The expected bytes of nxg_encode_clients, from the CPU oracle (test infrastructure).

Client c's payload is what the oracle's encoder writes for the batch's rows gathered by
ent_row[chan_off[c]:chan_off[c+1]]. The children arrays stay the batch's, unchanged: the oracle
addresses an Array's, Map's or Error's elements at cfixed[fixed + i], so gathered rows may share
children. client_off is the running sum of the payload lengths.
"""
import numpy as np

import nxo


def client_payload(cols, heap, rows):
    """nxo.encode of the batch's rows `rows` (any order, repeats allowed). cols: dict with id,
    tag, fixed, aux and optionally ctag, cfixed, caux (numpy)."""
    rows = np.asarray(rows, np.int64)
    ctag = cols.get("ctag")
    nc = 0 if ctag is None else len(ctag)
    d = nxo.Decoded(max(len(rows), 1), max(nc, 1), 1)
    n = len(rows)
    d.id[:n] = cols["id"][rows]
    d.tag[:n] = cols["tag"][rows]
    d.fixed[:n] = cols["fixed"][rows]
    d.aux[:n] = cols["aux"][rows]
    if nc:
        d.ctag[:nc], d.cfixed[:nc], d.caux[:nc] = ctag, cols["cfixed"], cols["caux"]
    d.s.n_rows, d.s.n_children, d.s.n_ctl = n, nc, 0
    return nxo.encode(d, heap if heap is not None and len(heap) else np.zeros(1, np.uint8))


def expected(cols, heap, chan_off, ent_row):
    """(bytes, client_off[n_clients + 1] as uint64) of the whole call. Entries before chan_off[0]
    (none in a dispatch) would lie in front of client 0's payload; the model takes chan_off[0] = 0."""
    chan_off = np.asarray(chan_off, np.int64)
    ent_row = np.asarray(ent_row, np.int64)
    assert chan_off[0] == 0 and np.all(np.diff(chan_off) >= 0)
    parts, off = [], [0]
    for c in range(len(chan_off) - 1):
        seg = ent_row[chan_off[c]:chan_off[c + 1]]
        p = client_payload(cols, heap, seg) if len(seg) else b""
        parts.append(p)
        off.append(off[-1] + len(p))
    return b"".join(parts), np.array(off, np.uint64)


def f64_cols(ids, bits):
    """F64-layout columns (id, the f64's bits) as the mixed columns the oracle encodes."""
    n = len(ids)
    return {"id": np.asarray(ids, np.uint64), "tag": np.full(n, 9, np.uint8),
            "fixed": np.asarray(bits, np.uint64), "aux": np.zeros(n, np.uint32)}
