"""The sequential model of nxg_archive_decode_window and nxg_archive_build_image
(include/nxg_codec.h) -- TEST INFRASTRUCTURE.

The window: the oracle's archive decoder (nxo.decode_archive) once per record, the results
concatenated in record order with text offsets moved by the record's place in the buffer and
child indices moved by the running child count. A record that fails contributes no rows and keeps
its (err_kind, err_offset). The image: a Python dict fold in row order (HashMap::extend,
netidx-archive/src/logfile/reader.rs:519-552), sorted by Id."""
import numpy as np

import nxo

HEAP_TAGS = (12, 13, 18, 20, 27)   # fixed = the payload's offset in the heap
CONTAINER_TAGS = (19, 21, 22)      # fixed = the first child slot
ROW_COLS = ("id", "tag", "fixed", "aux")
CHILD_COLS = ("ctag", "cfixed", "caux")
INFO = ("row_off", "n_rows", "child_off", "n_children", "consumed", "err_kind", "err_offset")


def _rebase(tag, fixed, text_off, child_off):
    f = fixed.astype(np.uint64).copy()
    f[np.isin(tag, HEAP_TAGS)] += np.uint64(text_off)
    f[np.isin(tag, CONTAINER_TAGS)] += np.uint64(child_off)
    return f


def window(buf, recs):
    """buf: the whole buffer (uint8 array); recs: [(out_off, out_len[, err])]. Returns (columns
    dict, [info dict per record])."""
    parts = {k: [] for k in ROW_COLS + CHILD_COLS}
    infos = []
    rows = kids = 0
    for r in recs:
        off, ln = int(r[0]), int(r[1])
        skip = len(r) > 2 and r[2]
        f = dict.fromkeys(INFO, 0)
        f["row_off"], f["child_off"] = rows, kids
        if not skip:
            d, used = nxo.decode_archive(buf[off:off + ln])
            o = d.trim()
            if o["err_kind"]:
                f["err_kind"], f["err_offset"] = int(o["err_kind"]), int(o["err_offset"])
            else:
                f["n_rows"], f["n_children"], f["consumed"] = len(o["id"]), len(o["ctag"]), used
                parts["id"].append(o["id"])
                parts["tag"].append(o["tag"])
                parts["fixed"].append(_rebase(o["tag"], o["fixed"], off, kids))
                parts["aux"].append(o["aux"])
                parts["ctag"].append(o["ctag"])
                parts["cfixed"].append(_rebase(o["ctag"], o["cfixed"], off, kids))
                parts["caux"].append(o["caux"])
                rows += f["n_rows"]
                kids += f["n_children"]
        infos.append(f)
    dt = {"id": np.uint64, "tag": np.uint8, "fixed": np.uint64, "aux": np.uint32,
          "ctag": np.uint8, "cfixed": np.uint64, "caux": np.uint32}
    cols = {k: (np.concatenate(v).astype(dt[k]) if v else np.zeros(0, dt[k]))
            for k, v in parts.items()}
    return cols, infos


def image(cols, n_ids, keep=None):
    """The fold of build_image over the window's rows: {id: last row}, rows of Ids with
    keep[id] == 0 dropped. Returns (dict of id/tag/fixed/aux/src_row sorted by Id, n_filtered);
    ValueError naming the Id and the row when an Id is >= n_ids."""
    last = {}
    dropped = 0
    for row, i in enumerate(cols["id"].tolist()):
        if i >= n_ids:
            raise ValueError(f"Id {i} at row {row}")
        if keep is not None and not keep[i]:
            dropped += 1
            continue
        last[i] = row
    ids = sorted(last)
    src = np.array([last[i] for i in ids], np.uint64)
    s = src.astype(np.int64)
    return {"id": np.array(ids, np.uint64), "tag": cols["tag"][s], "fixed": cols["fixed"][s],
            "aux": cols["aux"][s], "src_row": src}, dropped


def reference_fold(batches, keep=None):
    """reader.rs:519-552 restated directly: `image.extend(batch.iter().filter_map(|BatchItem(id,
    up)| if filter.contains(id) { Some((*id, up.clone())) } else { None }))` over the batches in
    order. batches: lists of (id, event); keep: a set of Ids or None (no filter). Returns the map."""
    img = {}
    for batch in batches:
        img.update((i, ev) for i, ev in batch if keep is None or i in keep)
    return img


def value(tag, fixed, aux, ch, heap):
    """The Value of one slot as a nested tuple (text by content, containers by their elements),
    so that columns with different heaps and child layouts compare."""
    tag, fixed, aux = int(tag), int(fixed), int(aux)
    if tag in HEAP_TAGS:
        return (tag, bytes(heap[fixed:fixed + aux]))
    if tag in CONTAINER_TAGS:
        n = aux if tag == 19 else (2 * aux if tag == 21 else 1)
        return (tag, tuple(value(ch["ctag"][j], ch["cfixed"][j], ch["caux"][j], ch, heap)
                           for j in range(fixed, fixed + n)))
    return (tag, fixed, aux)


def values(rows, ch, heap):
    """[(id, value)] of row columns `rows` with children `ch` and text at `heap`."""
    return [(int(i), value(t, f, a, ch, heap))
            for i, t, f, a in zip(rows["id"], rows["tag"], rows["fixed"], rows["aux"])]
