"""The per-client encode's case table and model, on the CPU.

Every case of tests/client_frames_cases.py sits in the branch it is named for (the tile sizes and
staging bounds are read from the kernel sources, so a retune names the case that moved), and the
model of tests/client_frames_model.py is held to an independent restatement: for rows of scalars
and text, a client's payload is the concatenation of netidx_amd.msg_update over its entries."""
import numpy as np
import pytest

import netidx_amd
import client_frames_cases as cfc
import client_frames_model as model

LAYOUTS = ("f64", "mixed")


def test_constants_read_from_the_kernels():
    k = cfc.constants()
    assert k["T_MIXED"] == k["TPB"] * k["GRPT"] and k["T_F64"] == k["F64_TPB"] * k["RPT"]
    assert k["T_MIXED"] >= 64 and k["T_F64"] >= 64


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_case_sits_in_its_branch(layout):
    T = cfc.tile_size(layout)
    cs = cfc.cases(layout)
    for E in (0, 1, 2, T - 1, T, T + 1, 2 * T + 3):
        assert f"count_{E}" in cs
    for nc in (1, 2, 1025, 70000):
        assert cs[f"clients_{nc}"].n_clients == nc
        assert cs[f"clients_{nc}"].n_clients >= 1 and len(cs[f"clients_{nc}"].ent_row) == 300
    for name, c in cs.items():
        p = cfc.plan(c, layout)
        w = c.want
        if "ntiles" in w:
            assert p.ntiles == w["ntiles"], (name, p.ntiles)
        if "staged" in w:
            assert [t.staged for t in p.tiles] == w["staged"], (name, [t.bytes for t in p.tiles])
        for cl, tile in w.get("first_in_tile", {}).items():
            assert cl in p.tiles[tile].clients, (name, cl, tile)
        # every client's offset is stored by exactly one tile
        if p.ntiles:
            owners = np.concatenate([t.clients for t in p.tiles])
            assert sorted(owners.tolist()) == list(range(c.n_clients + 1)), name
    # the named edges
    e = cs["edges"]
    assert set(e.chan_off.tolist()) >= {T - 1, T, T + 1}
    r = cs["empty_runs"].chan_off.tolist()
    assert r[:4] == [0] * 4 and r[5:9] == [T] * 4 and r[9:13] == [T + 7] * 4 and len(set(r[13:])) == 1
    assert sorted(set(cs["varint_ids"].cols["id"].tolist())) == sorted(cfc.VARINT_IDS)
    assert np.all(np.diff(cs["descending"].ent_row.astype(np.int64)) == -1)
    assert len(set(cs["one_row_3000"].ent_row.tolist())) == 1
    if layout == "mixed":
        lm = cs["long_messages"]
        assert set(cfc.TEXT_LENS) | {cfc.BIG_BYTES} <= set(lm.cols["aux"].tolist())
        big = int(np.flatnonzero(lm.cols["aux"] == cfc.BIG_BYTES)[0])
        assert lm.ent_row[T - 1:T + 2].tolist() == [big] * 3


def restated(case):
    """The payloads from netidx_amd.msg_update alone."""
    c = case.cols
    parts, off = [], [0]
    for cl in range(case.n_clients):
        b = bytearray()
        for r in case.ent_row[int(case.chan_off[cl]):int(case.chan_off[cl + 1])].tolist():
            tag, fixed, aux = int(c["tag"][r]), int(c["fixed"][r]), int(c["aux"][r])
            text = bytes(case.heap[fixed:fixed + aux]) if tag in (12, 13) else b""
            b += netidx_amd.msg_update(int(c["id"][r]), tag, fixed, aux, text)
        parts.append(bytes(b))
        off.append(off[-1] + len(b))
    return b"".join(parts), np.array(off, np.uint64)


@pytest.mark.parametrize("layout,name", [
    ("f64", "count_1"), ("f64", "varint_ids"), ("f64", "shared_rows"), ("f64", "clients_1025"),
    ("mixed", "edges"), ("mixed", "empty_runs"), ("mixed", "long_messages"), ("mixed", "overflow"),
])
def test_model_matches_restatement(layout, name):
    case = cfc.cases(layout)[name]
    want, woff = restated(case)
    got, goff = model.expected(case.cols, case.heap, case.chan_off, case.ent_row)
    assert np.array_equal(goff, woff)
    assert got == want
    # and the lengths plan() works from
    assert int(cfc.msg_lens(case).sum()) == len(want)
