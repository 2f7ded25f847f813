#!/usr/bin/env python3
"""Timing of the value table (nxg_value_table_apply / _rebuild) against what a caller had to do
before it. Shapes:
  1  an F64 table of N slots, every slot updated from the bench's commit shape (N f64 rows)
  2  config 3's mixed columns as N slots, every slot updated
  3  the same table, 1 % of the slots updated
  4  a forced rebuild of (2)
  5  10^4 slots of 100 KB Abstracts, every slot updated
Baselines, in the same process and alternated with the call: for (1) the torch expression
cur_fixed[m] = fixed[last_row[m] - 1]; for (2)-(5) the batch's columns and last_row copied to the
host, folded into a rebuilt (compacted) table with numpy, and that table uploaded. Before timing,
the numpy fold must equal nxg_value_table_rebuild of the same inputs byte for byte (rows, heap,
children), and the apply's rows must carry the same tags, lengths and live totals; (1) must equal
the torch result. Windows of at least 0.25 s of calls, each ending in a device synchronise;
medians of 7. An apply appends, so the table is re-initialised and re-populated (untimed) whenever
the next apply would not fit.
usage: python3 scripts/value_table_measure.py [--n 10000000] [--shapes 1,2,3,4,5] [--only-a]
--only-a: the checks and three calls per shape, no baseline, for a separate `rocprofv3
--kernel-trace --stats` run (its kernel_stats.csv gives the per-kernel times); every line states
the shape's algorithmic bytes, computed here from the shapes, to put beside them."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

def numpy_fold(np, cur, batch, last_row):
    """The rebuilt table (flat values only: text, Decimal, Abstract, arrays of scalars): rows,
    heap and children compacted in slot order."""
    n = len(cur["fixed"])
    sel = np.flatnonzero(last_row)
    r = (last_row[sel] - 1).astype(np.int64)
    tag, aux = cur["tag"].copy(), cur["aux"].copy()
    tag[sel], aux[sel] = batch["tag"][r], batch["aux"][r]
    src = cur["fixed"].astype(np.int64)
    is_text = np.isin(tag, (12, 13, 18, 27))
    is_arr = tag == 19
    bsrc = batch["fixed"][r].astype(np.int64)
    bt = batch["tag"][r]
    # batch payloads live behind the table's in one concatenated source
    bsrc = np.where(np.isin(bt, (12, 13, 18, 20, 27)), bsrc + len(cur["heap"]),
                    np.where(bt == 19, bsrc + len(cur["ctag"]), bsrc))
    src[sel] = bsrc
    blen = np.where(is_text, aux, np.where(tag == 20, 16, 0)).astype(np.int64)
    klen = np.where(is_arr, aux, 0).astype(np.int64)
    hoff = np.cumsum(blen) - blen
    koff = np.cumsum(klen) - klen
    H = np.concatenate([cur["heap"], batch["heap"]])
    nb, nk = int(blen.sum()), int(klen.sum())
    if nb and nb / max(int((blen > 0).sum()), 1) > 4096:  # long payloads: one copy each
        heap = np.empty(nb, np.uint8)
        for s in np.flatnonzero(blen).tolist():
            heap[hoff[s]:hoff[s] + blen[s]] = H[src[s]:src[s] + blen[s]]
    else:
        heap = H[np.repeat(src - hoff, blen) + np.arange(nb)]
    kidx = np.repeat(src - koff, klen) + np.arange(nk)
    out = {"tag": tag, "aux": aux, "heap": heap}
    for k in ("ctag", "cfixed", "caux"):
        out[k] = np.concatenate([cur[k], batch[k]])[kidx]
    fx = np.where(blen > 0, hoff, np.where(is_arr, koff, src))  # (all int64: no float promotion)
    out["fixed"] = np.where(is_text & (blen == 0), hoff, fx).astype(np.uint64)
    return out


def main():
    import numpy as np
    import torch
    import netidx_amd
    from netidx_amd import synth
    from netidx_amd.codec import ValueTable

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--shapes", default="1,2,3,4,5")
    ap.add_argument("--only-a", action="store_true")
    args = ap.parse_args()
    n = args.n
    shapes = [int(x) for x in args.shapes.split(",")]
    codec = netidx_amd.Codec(0)
    cu = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a).view(dt) if dt else a).cuda()

    def window(fn, reset=None):
        """ms per call over at least 0.25 s of calls; reset() (untimed) returns False when the
        next call needs a fresh table."""
        total, k = 0.0, 0
        while total < 0.25:
            if reset is not None:
                reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            total += time.perf_counter() - t0
            k += 1
        return total / k * 1e3

    def report(shape, what, run_a, run_b, algo, reset=None, **kw):
        if args.only_a:
            for _ in range(3):
                if reset is not None:
                    reset()
                run_a()
            torch.cuda.synchronize()
            print(json.dumps(dict(shape=shape, what=what, only_a=True, algorithmic_bytes=algo,
                                  **kw)), flush=True)
            return
        ta, tb = [], []
        for _ in range(7):
            ta.append(window(run_a, reset))
            tb.append(window(run_b))
        ma, mb = statistics.median(ta), statistics.median(tb)
        print(json.dumps(dict(shape=shape, what=what, a_ms=round(ma, 4), b_ms=round(mb, 4),
                              a_range=[round(min(ta), 4), round(max(ta), 4)],
                              b_range=[round(min(tb), 4), round(max(tb), 4)],
                              b_over_a=round(mb / ma, 2), algorithmic_bytes=algo,
                              a_call_share_of_8TBps=round(algo / (ma * 1e-3) / 8e12, 4), **kw)),
              flush=True)

    if 1 in shapes:  # ---- an F64 table, every slot from a commit of n f64 rows
        ids, vals = synth.f64_columns(n)
        batch = netidx_amd.columns_from_arrays(ids, vals)
        rng = np.random.default_rng(1)
        last = cu((rng.permutation(n) + 1).astype(np.int64))
        vt = ValueTable(codec, n, f64=True).init()
        cur = torch.zeros(n, dtype=torch.int64, device="cuda")
        m = last != 0

        def a1():
            vt.apply(batch, last)

        def b1():
            cur[m] = batch.fixed[:n][last[m] - 1]

        a1()
        b1()
        torch.cuda.synchronize()
        assert torch.equal(cur, vt.t["fixed"][:n]), "shape 1 differs"
        report(1, "f64 table, all slots", a1, b1, 8 * n + 8 * n + 8 * n, n=n)
        del vt, cur, batch, last

    def mixed_case(mc_np, frac):
        """(ValueTable populated from mc_np, batch columns, heap, last_row, host copies)."""
        N = len(mc_np.id)
        batch = netidx_amd.columns_from_arrays(mc_np.id, mc_np.fixed, mc_np.tag, mc_np.aux,
                                               mc_np.ctag, mc_np.cfixed, mc_np.caux)
        heap = cu(mc_np.heap.copy())
        hb, kb = len(mc_np.heap), len(mc_np.ctag)
        rng = np.random.default_rng(2)
        lr = (rng.permutation(N) + 1).astype(np.int64)
        if frac < 1:
            lr[rng.random(N) >= frac] = 0
        return batch, heap, cu(lr), lr.astype(np.uint64), hb, kb

    def run_mixed(shape, what, mc_np, frac, rebuild=False):
        N = len(mc_np.id)
        batch, heap, last, lr, hb, kb = mixed_case(mc_np, frac)
        ident = cu(np.arange(1, N + 1, dtype=np.int64))
        reps = 4
        vt = ValueTable(codec, N, reps * hb + 16, reps * kb + 16)

        def populate():
            vt.init()
            vt.apply(batch, ident, heap)

        populate()
        host = vt.numpy()
        cur = {k: host[k] for k in ("tag", "fixed", "aux", "heap", "ctag", "cfixed", "caux")}
        hbatch = dict(tag=mc_np.tag, fixed=mc_np.fixed, aux=mc_np.aux, heap=mc_np.heap,
                      ctag=mc_np.ctag, cfixed=mc_np.cfixed, caux=mc_np.caux)
        dst = ValueTable(codec, N, hb + 16, kb + 16)
        # equality before timing: numpy fold == device rebuild; apply: same rows and live totals
        want = numpy_fold(np, cur, hbatch, lr)
        vt.rebuild(dst, batch, last, heap)
        got = dst.numpy()
        for k in ("tag", "fixed", "aux", "heap", "ctag", "cfixed", "caux"):
            assert np.array_equal(got[k], want[k]), (shape, k)
        res = vt.apply(batch, last, heap)
        after = vt.numpy()
        assert np.array_equal(after["tag"], want["tag"]) and np.array_equal(after["aux"],
                                                                            want["aux"])
        assert (res["live_bytes"], res["live_children"]) == (len(want["heap"]), len(want["ctag"]))
        need_b, need_k = res["need_bytes"], res["need_children"]
        populate()

        def reset():
            if (vt.heap_used + need_b > vt.s.cap_bytes or
                    vt.child_used + need_k > vt.s.cap_children):
                populate()

        def a():
            if rebuild:
                vt.rebuild(dst, batch, last, heap)
            else:
                vt.apply(batch, last, heap)

        up = {}

        def b():
            h = {k: getattr(batch, k)[:N].cpu().numpy() for k in ("tag", "fixed", "aux")}
            h["fixed"] = h["fixed"].view(np.uint64)
            h["aux"] = h["aux"].view(np.uint32)
            h["heap"] = heap.cpu().numpy()
            for k in ("ctag", "cfixed", "caux"):
                h[k] = getattr(batch, k)[:kb].cpu().numpy()
            h["cfixed"], h["caux"] = h["cfixed"].view(np.uint64), h["caux"].view(np.uint32)
            l = last.cpu().numpy().view(np.uint64)
            w = numpy_fold(np, cur, h, l)
            for k, v in w.items():
                up[k] = torch.from_numpy(np.ascontiguousarray(v).view(
                    {8: np.int64, 4: np.int32, 1: np.uint8}[v.dtype.itemsize])).cuda()

        nsel = int((lr != 0).sum())
        # src_row, the per-slot scratch both passes touch, the selected rows' columns, the new rows,
        # payload bytes and child slots read and written
        algo = 8 * N + 2 * 24 * N + 13 * nsel + 13 * nsel + 2 * need_b + 2 * 13 * need_k
        if rebuild:
            algo += 13 * (N - nsel)
        report(shape, what, a, b, algo, None if rebuild else reset, n=N, selected=nsel,
               need_bytes=need_b, need_children=need_k)

    if any(s in shapes for s in (2, 3, 4)):
        m = synth.mixed_columns(n)
        if 2 in shapes:
            run_mixed(2, "mixed table, all slots", m, 1.0)
        if 3 in shapes:
            run_mixed(3, "mixed table, 1 % of the slots", m, 0.01)
        if 4 in shapes:
            run_mixed(4, "forced rebuild of (2)", m, 1.0, rebuild=True)
    if 5 in shapes:
        from collections import namedtuple
        N, L = 10_000, 100_000
        MC = namedtuple("MC", "id tag fixed aux ctag cfixed caux heap")
        rng = np.random.default_rng(5)
        mc = MC(np.arange(N, dtype=np.uint64), np.full(N, 27, np.uint8),
                (np.arange(N, dtype=np.uint64) * np.uint64(L)), np.full(N, L, np.uint32),
                np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32),
                rng.integers(0, 256, N * L, dtype=np.uint8))
        run_mixed(5, "10^4 Abstracts of 100 KB", mc, 1.0)
    codec.close()


if __name__ == "__main__":
    main()
