"""The models of nxg_replay_window and nxg_replay_image (include/nxg_codec.h) -- TEST
INFRASTRUCTURE. Two independent restatements each:

  window_loop / image_loop    the reference's loops line by line (process_batch, netidx-archive/src/
                              recorder/publish/session_shard.rs:196-245; reimage, :375-409) with a
                              dict for `published`, one item at a time
  window_numpy / image_numpy  the same results from whole-array numpy operations

and the plain reference playback (`reference_playback`) against which the stop protocol
(`protocol_playback`) is compared: a model publisher that assigns Ids as paths are published.

A window is a dict of numpy columns (id, tag, fixed, aux), `infos` a list of (row_off, n_rows),
`table` the uint64 array pub_id_of_arch. Results are `Result`s."""
import numpy as np

DROP = 0xFFFFFFFFFFFFFFFF
MISS = 0xFFFFFFFFFFFFFFFE
U64_MAX = 0xFFFFFFFFFFFFFFFF
TAG_UNSUB = 0x40
TAG_NULL = 16
ROW_COLS = ("id", "tag", "fixed", "aux", "src_row")
DT = {"id": np.uint64, "tag": np.uint8, "fixed": np.uint64, "aux": np.uint32,
      "src_row": np.uint64}


class Result:
    """rows: dict of the five row arrays; rec_off (uint64, n_recs + 1); n_dropped, n_done, n_miss;
    miss: every miss row of the stopping record (the call lists the first cap_miss of them)."""

    def __init__(self, rows, rec_off, n_dropped, n_done, miss):
        self.rows = {k: np.asarray(rows[k], DT[k]) for k in ROW_COLS}
        self.rec_off = np.asarray(rec_off, np.uint64)
        self.n_rows = len(self.rows["id"])
        self.n_dropped, self.n_done = int(n_dropped), int(n_done)
        self.miss = np.asarray(miss, np.uint64)
        self.n_miss = len(self.miss)

    def same(self, o):
        return (all(np.array_equal(self.rows[k], o.rows[k]) for k in ROW_COLS)
                and np.array_equal(self.rec_off, o.rec_off)
                and (self.n_dropped, self.n_done) == (o.n_dropped, o.n_done)
                and np.array_equal(self.miss, o.miss))


def _rows(lst):
    return {k: np.array([r[j] for r in lst], DT[k]) for j, k in enumerate(ROW_COLS)}


# ---- the reference's loops --------------------------------------------------------------------------
def window_loop(cols, infos, table):
    """process_batch per record, stopping in front of the first record that would publish."""
    published = {a: int(p) for a, p in enumerate(table.tolist()) if p not in (DROP, MISS)}
    wanted = {a for a, p in enumerate(table.tolist()) if p == MISS}  # a path the filter matches
    n_ids = len(table)
    out, rec_off, dropped, n_done, miss = [], [0], 0, len(infos), []
    for i, (off, n) in enumerate(infos):
        pbatch, drops, must_publish = [], 0, []
        for r in range(off, off + n):
            a = int(cols["id"][r])
            if int(cols["tag"][r]) == TAG_UNSUB:      # Event::Unsubscribed => Value::Null
                v = (TAG_NULL, 0, 0)
            else:                                      # Event::Update(v) => v
                v = (int(cols["tag"][r]), int(cols["fixed"][r]), int(cols["aux"][r]))
            if a in published:                         # Some(val) => val.update(&mut pbatch, v)
                pbatch.append((published[a],) + v + (r,))
            elif a >= n_ids or a in wanted:            # None => path_for_id: the host publishes
                must_publish.append(r)
            else:                                      # no path / filter mismatch: dropped
                drops += 1
        if must_publish:
            n_done, miss = i, must_publish
            break
        out += pbatch                                  # pbatch.commit
        dropped += drops
        rec_off.append(len(out))
    rec_off += [len(out)] * (len(infos) + 1 - len(rec_off))
    return Result(_rows(out), rec_off, dropped, n_done, miss)


def image_loop(image, order, table):
    """reimage: every Id of the pathmap gets its image value, or Null."""
    img = {int(i): k for k, i in enumerate(image["id"].tolist())}
    n_ids = len(table)
    out, dropped, miss = [], 0, []
    for j, a in enumerate(int(x) for x in order):
        p = int(table[a]) if a < n_ids else MISS
        if p == MISS:
            miss.append(j)
        elif p == DROP:
            dropped += 1
        else:
            k = img.get(a)
            if k is None or int(image["tag"][k]) == TAG_UNSUB:
                out.append((p, TAG_NULL, 0, 0, U64_MAX))
            else:
                out.append((p, int(image["tag"][k]), int(image["fixed"][k]),
                            int(image["aux"][k]), k))
    return Result(_rows(out), [0, len(out)], dropped, 1, miss)


# ---- the same, vectorised ----------------------------------------------------------------------------
def _lookup(ids, table):
    ids = np.asarray(ids, np.uint64)
    inside = ids < np.uint64(len(table))
    p = np.full(len(ids), MISS, np.uint64)
    p[inside] = np.asarray(table, np.uint64)[ids[inside].astype(np.int64)]
    return p


def window_numpy(cols, infos, table):
    n_recs = len(infos)
    off = np.array([f[0] for f in infos], np.int64).reshape(-1)
    cnt = np.array([f[1] for f in infos], np.int64).reshape(-1)
    total = int(cnt.sum())
    rec = np.repeat(np.arange(n_recs), cnt)
    r = (np.repeat(off, cnt) + np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt)).astype(np.int64)
    p = _lookup(cols["id"][r], table)
    is_miss, is_drop = p == np.uint64(MISS), p == np.uint64(DROP)
    n_done = int(rec[is_miss].min()) if is_miss.any() else n_recs
    live = rec < n_done
    kept = live & ~is_miss & ~is_drop
    rk = r[kept]
    unsub = cols["tag"][rk] == TAG_UNSUB
    rows = {"id": p[kept], "tag": np.where(unsub, TAG_NULL, cols["tag"][rk]),
            "fixed": np.where(unsub, 0, cols["fixed"][rk]),
            "aux": np.where(unsub, 0, cols["aux"][rk]), "src_row": rk}
    per_rec = np.bincount(rec[kept], minlength=n_recs) if n_recs else np.zeros(0, np.int64)
    rec_off = np.concatenate([[0], np.cumsum(per_rec)])
    miss = r[is_miss & (rec == n_done)]
    return Result(rows, rec_off, int((live & is_drop).sum()), n_done, miss)


def image_numpy(image, order, table):
    order = np.asarray(order, np.uint64)
    p = _lookup(order, table)
    is_miss, is_drop = p == np.uint64(MISS), p == np.uint64(DROP)
    kept = ~is_miss & ~is_drop
    a = order[kept]
    ids = np.asarray(image["id"], np.uint64)
    k = np.searchsorted(ids, a)
    kc = np.minimum(k, max(len(ids) - 1, 0))
    have = (k < len(ids)) & (ids[kc] == a if len(ids) else np.zeros(len(a), bool))
    if len(ids):
        have &= image["tag"][kc] != TAG_UNSUB
        tag, fixed, aux = image["tag"][kc], image["fixed"][kc], image["aux"][kc]
    else:
        tag = fixed = aux = np.zeros(len(a), np.uint64)
    rows = {"id": p[kept], "tag": np.where(have, tag, TAG_NULL), "fixed": np.where(have, fixed, 0),
            "aux": np.where(have, aux, 0),
            "src_row": np.where(have, kc.astype(np.uint64), np.uint64(U64_MAX))}
    n = int(kept.sum())
    return Result(rows, [0, n], int(is_drop.sum()), 1, np.flatnonzero(is_miss))


# ---- playback against a model publisher ----------------------------------------------------------
class Publisher:
    """Assigns publisher Ids from a counter as paths are published; `current` per Id."""

    def __init__(self, next_id=100):
        self.next_id, self.current = next_id, {}

    def publish(self, v):
        i = self.next_id
        self.next_id += 1
        self.current[i] = v
        return i

    def commit(self, updates):
        for i, v in updates:
            self.current[i] = v


def _value(cols, r):
    if int(cols["tag"][r]) == TAG_UNSUB:
        return (TAG_NULL, 0, 0)
    return (int(cols["tag"][r]), int(cols["fixed"][r]), int(cols["aux"][r]))


def reference_playback(cols, infos, published, has_path):
    """process_batch over every record, publishing where the reference publishes. published:
    {archive Id: publisher Id} (copied); has_path: the archive Ids with a path the filter matches.
    Returns ([(publishes, updates) per record], publisher): publishes [(archive Id, pub Id,
    value)], updates [(pub Id, value)], each in item order."""
    pub = Publisher()
    published = dict(published)
    log = []
    for off, n in infos:
        publishes, updates = [], []
        for r in range(off, off + n):
            a, v = int(cols["id"][r]), _value(cols, r)
            if a in published:
                updates.append((published[a], v))
            elif a in has_path:
                published[a] = pub.publish(v)
                publishes.append((a, published[a], v))
        pub.commit(updates)
        log.append((publishes, updates))
    return log, pub


def protocol_playback(cols, infos, published, has_path, n_ids, cap_miss, replay=window_loop):
    """The same playback through the stop protocol: replay, publish the listed misses (first row
    per Id), update the table, call again from record n_done. The row that published comes back as
    an Update of the value that is already `current`: it is checked to be exactly that and left
    out of the log, since neither a client's bytes nor `current` change by it. Returns (log,
    publisher, calls)."""
    pub = Publisher()
    table = np.full(n_ids, DROP, np.uint64)
    for a in has_path:
        if a < n_ids:
            table[a] = MISS
    for a, p in published.items():
        table[a] = p
    log = [([], []) for _ in infos]
    redundant = set()
    start = calls = 0
    while True:
        res = replay(cols, infos[start:], table)
        calls += 1
        for i in range(res.n_done):
            lo, hi = int(res.rec_off[i]), int(res.rec_off[i + 1])
            ups = []
            for k in range(lo, hi):
                p, r = int(res.rows["id"][k]), int(res.rows["src_row"][k])
                v = (int(res.rows["tag"][k]), int(res.rows["fixed"][k]), int(res.rows["aux"][k]))
                if r in redundant:
                    assert pub.current[p] == v, "the publishing row is not an Update of `current`"
                    redundant.discard(r)
                    continue
                ups.append((p, v))
            pub.commit(ups)
            log[start + i][1].extend(ups)
        start += res.n_done
        if start == len(infos):
            return log, pub, calls
        for r in res.miss[:cap_miss].tolist():
            a = int(cols["id"][r])
            if a >= n_ids:  # an Id past the table: the host grows it from what it knows
                grown = np.full(a + 1 - n_ids, DROP, np.uint64)
                for b in has_path:
                    if n_ids <= b <= a:
                        grown[b - n_ids] = MISS
                table = np.concatenate([table, grown])
                n_ids = a + 1
            if table[a] != np.uint64(MISS):
                continue  # published by an earlier row of this list, or no path after all
            v = _value(cols, r)
            table[a] = pub.publish(v)
            log[start][0].append((a, int(table[a]), v))
            redundant.add(r)
