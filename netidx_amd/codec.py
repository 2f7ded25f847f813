"""ctypes binding of the C ABI in include/nxg_codec.h (netidx_amd/lib/libnxg_codec.so).

The Python surface mirrors the two seams that the codec replaces in the reference:

* ``Codec.decode_batch(frame)`` replaces the ``decode_task`` -> ``receive_batch_fn`` loop
  (netidx/src/subscriber/connection.rs:209-242, netidx/src/channel.rs:504-521). A malformed
  frame raises ``PackError`` with the reference's kind and the offset of the first failing
  message, and the whole frame is rejected, as in connection.rs:228-231.
* ``Codec.encode_batch(cols)`` replaces the ``handle_updates`` -> ``queue_send`` loop
  (netidx/src/publisher/server.rs:610-612, netidx/src/channel.rs:177-202).
* ``Codec.decode_writes(frame)`` / ``Codec.encode_writes(cols, wcols)`` are the other direction,
  publisher::To: the publisher's ``con.receive_batch`` (publisher/server.rs:660) and the
  subscriber's ``queue_send(&To::Write(..))`` loop (subscriber/connection.rs:384-399).

The product path is the HIP library. There is no CPU fallback: if the shared library or a GPU
is missing, the calls raise.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# NXG_LIB: another build of the same library (A/B experiments, scripts/ab_variants.sh)
LIB_PATH = os.environ.get("NXG_LIB") or os.path.join(HERE, "lib", "libnxg_codec.so")

# NxgErrKind (include/nxg_codec.h) = PackError (netidx-core/src/pack.rs:89-95) + codec kinds
OK, UNKNOWN_TAG, TOO_BIG, INVALID_FORMAT, BUFFER_SHORT = 0, 1, 2, 3, 4
DEPTH, CAPACITY, NOT_F64, TIMEOUT = 6, 7, 8, 9
ERR_NAMES = {1: "UnknownTag", 2: "TooBig", 3: "InvalidFormat", 4: "BufferShort", 6: "Depth",
             7: "Capacity", 8: "NotF64", 9: "Timeout"}
LAYOUT_F64, LAYOUT_MIXED = 1, 2
MEM_DEVICE, MEM_HOST = 0, 1
HINT_MIXED = 1
# To frames (nxg_decode_writes): NxgWriteFlags and the status path
WRITE_REPLY, WRITE_NO_WID = 1, 2
PATH_WRITES = 6
PATH_WRITES_FAST = 8  # the fast To decoder took the frame (decode_writes(fast=True))


class PackError(Exception):
    """A frame the reference would reject (netidx-core/src/pack.rs:89-95)."""

    def __init__(self, kind, offset):
        self.kind = kind
        self.offset = offset
        super().__init__(f"{ERR_NAMES.get(kind, kind)} at message offset {offset}")


class CodecError(RuntimeError):
    """API misuse or a HIP failure (NetidxError)."""


class NetidxError(C.Structure):
    _fields_ = [("msg", C.c_char_p)]


U64P, U32P, U8P = C.c_void_p, C.c_void_p, C.c_void_p


class NxgColumns(C.Structure):
    _fields_ = [
        ("layout", C.c_uint32), ("mem", C.c_uint32),
        ("cap_rows", C.c_uint64), ("cap_children", C.c_uint64), ("cap_ctl", C.c_uint64),
        ("n_rows", C.c_uint64), ("n_children", C.c_uint64), ("n_ctl", C.c_uint64),
        ("n_heartbeat", C.c_uint64),
        ("id", C.c_void_p), ("tag", C.c_void_p), ("fixed", C.c_void_p), ("aux", C.c_void_p),
        ("ctag", C.c_void_p), ("cfixed", C.c_void_p), ("caux", C.c_void_p),
        ("ctl_row", C.c_void_p), ("ctl_off", C.c_void_p), ("ctl_len", C.c_void_p),
        ("ctl_variant", C.c_void_p),
    ]


class NxgWriteCols(C.Structure):
    _fields_ = [("mem", C.c_uint32), ("pad", C.c_uint32), ("cap_rows", C.c_uint64),
                ("wflags", C.c_void_p), ("wid", C.c_void_p)]


class NxgWriteDecodeOpts(C.Structure):
    _fields_ = [("fast", C.c_uint32), ("reserved", C.c_uint32)]


class NxgRange(C.Structure):
    _fields_ = [("begin", C.c_uint64), ("end", C.c_uint64), ("entry", C.c_uint64),
                ("exit", C.c_uint64), ("n_rows", C.c_uint64), ("ok", C.c_uint32),
                ("err_kind", C.c_uint32), ("err_offset", C.c_uint64)]

    def tuple(self):
        return (self.begin, self.end, self.entry, self.exit, self.n_rows, self.ok, self.err_kind,
                self.err_offset)

    @classmethod
    def of(cls, t):
        return cls(*t)


class NxgSubTable(C.Structure):
    _fields_ = [("n_ids", C.c_uint64), ("slot_of_id", C.c_void_p), ("n_slots", C.c_uint64),
                ("slot_sub_id", C.c_void_p), ("slot_stream_off", C.c_void_p),
                ("stream_chan", C.c_void_p), ("slot_has_last", C.c_void_p),
                ("n_chans", C.c_uint32)]


class NxgDispatch(C.Structure):
    _fields_ = [("cap_entries", C.c_uint64), ("chan_off", C.c_void_p), ("ent_sub", C.c_void_p),
                ("ent_row", C.c_void_p), ("last_row", C.c_void_p), ("n_entries", C.c_uint64),
                ("n_unmatched", C.c_uint64)]


class NxgClientFrames(C.Structure):
    _fields_ = [("cap_bytes", C.c_uint64), ("out", C.c_void_p), ("client_off", C.c_void_p),
                ("n_bytes", C.c_uint64)]


class NxgRecordTable(C.Structure):
    _fields_ = [("n_subs", C.c_uint64), ("arch_id_of_sub", C.c_void_p)]


class NxgRecordBatches(C.Structure):
    _fields_ = [("cap_bytes", C.c_uint64), ("out", C.c_void_p), ("rec_off", C.c_void_p),
                ("rec_items", C.c_void_p), ("n_bytes", C.c_uint64), ("n_items", C.c_uint64),
                ("n_dropped", C.c_uint64)]


class NxgArchiveIndexes(C.Structure):
    _fields_ = [("cap_bytes", C.c_uint64), ("out", C.c_void_p), ("idx_off", C.c_void_p),
                ("idx_ids", C.c_void_p), ("n_bytes", C.c_uint64), ("n_ids_total", C.c_uint64)]


INDEX_NONE, INDEX_MATCH, INDEX_ERR_SHORT, INDEX_ERR_FORMAT = 0, 1, 2, 3


class NxgOneshotPaths(C.Structure):
    _fields_ = [("n_ids", C.c_uint64), ("path_off", C.c_void_p), ("path_bytes", C.c_void_p)]


class NxgOneshotPathmap(C.Structure):
    _fields_ = [("cap_bytes", C.c_uint64), ("out", C.c_void_p), ("sel", C.c_void_p),
                ("n_bytes", C.c_uint64), ("n_sel", C.c_uint64)]


class NxgOneshotDeltas(C.Structure):
    _fields_ = [("cap_bytes", C.c_uint64), ("out", C.c_void_p), ("rec_off", C.c_void_p),
                ("rec_items", C.c_void_p), ("n_bytes", C.c_uint64), ("n_items", C.c_uint64),
                ("n_dropped", C.c_uint64), ("n_kept_recs", C.c_uint64)]


class NxgOneshotShardLayout(C.Structure):
    _fields_ = [("pathmap_len", C.c_uint64), ("image_len", C.c_uint64),
                ("deltas_len", C.c_uint64), ("n_deltas", C.c_uint64),
                ("pathmap_off", C.c_uint64), ("image_off", C.c_uint64),
                ("count_off", C.c_uint64), ("deltas_off", C.c_uint64), ("shard_len", C.c_uint64),
                ("len_head_len", C.c_uint32), ("count_head_len", C.c_uint32),
                ("len_head", C.c_uint8 * 10), ("count_head", C.c_uint8 * 10),
                ("pad", C.c_uint8 * 4)]


class NxgOneshotFrag(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("len", C.c_uint64)]


class NxgWriteTable(C.Structure):
    _fields_ = [("n_ids", C.c_uint64), ("perm_of_id", C.c_void_p), ("slot_of_id", C.c_void_p),
                ("n_slots", C.c_uint64), ("slot_chan_off", C.c_void_p), ("chan", C.c_void_p),
                ("n_chans", C.c_uint32)]


class NxgWriteRoute(C.Structure):
    _fields_ = [("cap_rows", C.c_uint64), ("outcome", C.c_void_p), ("disp", NxgDispatch),
                ("cap_wait", C.c_uint64), ("wait_row", C.c_void_p), ("wait_id", C.c_void_p),
                ("wait_wid", C.c_void_p), ("cap_unsub", C.c_uint64), ("unsub_id", C.c_void_p),
                ("cap_reply", C.c_uint64), ("reply", C.c_void_p),
                ("n_entries", C.c_uint64), ("n_wait", C.c_uint64), ("n_unsub", C.c_uint64),
                ("n_replies", C.c_uint64), ("reply_len", C.c_uint64), ("n_fresh", C.c_uint64),
                ("n_outcome", C.c_uint64 * 4), ("next_row", C.c_uint64),
                ("next_ctl", C.c_uint64), ("stopped_at_subscribe", C.c_uint32),
                ("pad", C.c_uint32)]


class NxgSubscribeTable(C.Structure):
    _fields_ = [("paths", C.c_void_p), ("pub", C.c_void_p), ("allow_of_id", C.c_void_p),
                ("n_defaults", C.c_uint64), ("default_heap", C.c_void_p),
                ("default_off", C.c_void_p), ("deferred_room", C.c_uint64)]


class NxgSubscribeRoute(C.Structure):
    _fields_ = [("cap_spans", C.c_uint64), ("outcome", C.c_void_p), ("span_id", C.c_void_p),
                ("cap_sub", C.c_uint64), ("sub_id", C.c_void_p), ("sub_perm", C.c_void_p),
                ("cap_deferred", C.c_uint64), ("deferred", C.c_void_p),
                ("cap_reply", C.c_uint64), ("reply", C.c_void_p),
                ("n_spans", C.c_uint64), ("n_sub", C.c_uint64), ("n_deferred", C.c_uint64),
                ("n_replies", C.c_uint64), ("reply_len", C.c_uint64),
                ("n_outcome", C.c_uint64 * 5), ("next_ctl", C.c_uint64),
                ("stopped", C.c_uint32), ("pad", C.c_uint32)]


class NxgReplyTable(C.Structure):
    _fields_ = [("subs", C.c_void_p), ("pending", C.c_void_p), ("n_pending", C.c_uint64),
                ("pend_slot", C.c_void_p), ("pend_alive", C.c_void_p)]


class NxgReplyRoute(C.Structure):
    _fields_ = [("cap_spans", C.c_uint64), ("outcome", C.c_void_p), ("span_q", C.c_void_p),
                ("span_id", C.c_void_p), ("disp", NxgDispatch),
                ("cap_sub", C.c_uint64), ("sub_span", C.c_void_p), ("sub_q", C.c_void_p),
                ("sub_id", C.c_void_p), ("cap_unsub", C.c_uint64), ("unsub_id", C.c_void_p),
                ("unsub_slot", C.c_void_p), ("cap_reply", C.c_uint64), ("reply", C.c_void_p),
                ("n_entries", C.c_uint64), ("n_sub", C.c_uint64), ("n_unsub", C.c_uint64),
                ("n_replies", C.c_uint64), ("reply_len", C.c_uint64),
                ("n_outcome", C.c_uint64 * 7), ("next_row", C.c_uint64),
                ("next_ctl", C.c_uint64), ("stopped", C.c_uint32), ("pad", C.c_uint32)]


TAG_BINS = 256


class NxgTagView(C.Structure):
    _fields_ = [("cap_rows", C.c_uint64), ("rank", C.c_void_p), ("row_of", C.c_void_p),
                ("fixed", C.c_void_p), ("aux", C.c_void_p), ("n_rows", C.c_uint64),
                ("count", C.c_uint64 * TAG_BINS), ("off", C.c_uint64 * (TAG_BINS + 1))]


class NxgPubTable(C.Structure):
    _fields_ = [("n_ids", C.c_uint64), ("slot_of_id", C.c_void_p), ("n_slots", C.c_uint64),
                ("slot_client_off", C.c_void_p), ("client", C.c_void_p), ("n_clients", C.c_uint32),
                ("cur_tag", C.c_void_p), ("cur_fixed", C.c_void_p), ("cur_aux", C.c_void_p),
                ("cur_heap", C.c_void_p), ("cur_ctag", C.c_void_p), ("cur_cfixed", C.c_void_p),
                ("cur_caux", C.c_void_p)]


class NxgValueTable(C.Structure):
    _fields_ = [("n_slots", C.c_uint64), ("tag", C.c_void_p), ("fixed", C.c_void_p),
                ("aux", C.c_void_p), ("heap", C.c_void_p), ("cap_bytes", C.c_uint64),
                ("ctag", C.c_void_p), ("cfixed", C.c_void_p), ("caux", C.c_void_p),
                ("cap_children", C.c_uint64), ("heap_used", C.c_uint64),
                ("heap_live", C.c_uint64), ("child_used", C.c_uint64),
                ("child_live", C.c_uint64)]


class NxgValueApply(C.Structure):
    _fields_ = [("n_applied", C.c_uint64), ("need_bytes", C.c_uint64),
                ("need_children", C.c_uint64), ("live_bytes", C.c_uint64),
                ("live_children", C.c_uint64)]

    def dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class NxgCtlMsg(C.Structure):
    _fields_ = [("msg_len", C.c_uint64), ("variant", C.c_uint32), ("permissions", C.c_uint32),
                ("id", C.c_uint64), ("path_off", C.c_uint64), ("path_len", C.c_uint64),
                ("timestamp", C.c_uint64), ("token_off", C.c_uint64), ("token_len", C.c_uint64),
                ("value_off", C.c_uint64), ("value_len", C.c_uint64), ("value_fixed", C.c_uint64),
                ("value_tag", C.c_uint32), ("value_aux", C.c_uint32)]


class NxgResolved(C.Structure):
    _fields_ = [("n_publishers", C.c_uint32), ("publisher_ipv4", C.c_uint32),
                ("publisher_id", C.c_uint64), ("publisher_port", C.c_uint16),
                ("resolver_port", C.c_uint16), ("resolver_ipv4", C.c_uint32),
                ("timestamp", C.c_uint64), ("flags", C.c_uint32), ("permissions", C.c_uint32)]


class NxgArchiveRecord(C.Structure):
    _fields_ = [("off", C.c_uint64), ("len", C.c_uint64), ("out_off", C.c_uint64),
                ("out_len", C.c_uint64), ("err", C.c_uint32), ("pad", C.c_uint32)]


class NxgArchiveBatchInfo(C.Structure):
    _fields_ = [("row_off", C.c_uint64), ("n_rows", C.c_uint64), ("child_off", C.c_uint64),
                ("n_children", C.c_uint64), ("consumed", C.c_uint64), ("err_kind", C.c_int32),
                ("path", C.c_uint32), ("err_offset", C.c_uint64)]

    FIELDS = ("row_off", "n_rows", "child_off", "n_children", "consumed", "err_kind", "path",
              "err_offset")

    def dict(self):
        return {k: int(getattr(self, k)) for k in self.FIELDS}


class NxgArchiveWindowOpts(C.Structure):
    _fields_ = [("big_record_bytes", C.c_uint64)]


class NxgZstdCompressOpts(C.Structure):
    _fields_ = [("literals", C.c_uint32), ("reserved", C.c_uint32 * 3)]


ZSTD_LIT_DICT_TREE, ZSTD_LIT_BLOCK_TREES = 0, 1


class NxgArchiveImage(C.Structure):
    _fields_ = [("cap_rows", C.c_uint64), ("id", C.c_void_p), ("tag", C.c_void_p),
                ("fixed", C.c_void_p), ("aux", C.c_void_p), ("src_row", C.c_void_p),
                ("n_rows", C.c_uint64), ("n_filtered", C.c_uint64)]


class NxgReplayTable(C.Structure):
    _fields_ = [("n_ids", C.c_uint64), ("pub_id_of_arch", C.c_void_p)]


class NxgReplayRows(C.Structure):
    _fields_ = [("cap_rows", C.c_uint64), ("id", C.c_void_p), ("tag", C.c_void_p),
                ("fixed", C.c_void_p), ("aux", C.c_void_p), ("src_row", C.c_void_p),
                ("rec_off", C.c_void_p), ("miss_row", C.c_void_p), ("cap_miss", C.c_uint64),
                ("n_rows", C.c_uint64), ("n_dropped", C.c_uint64), ("n_done", C.c_uint64),
                ("n_miss", C.c_uint64)]


REPLAY_DROP, REPLAY_MISS = 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFE


class NxgStatus(C.Structure):
    _fields_ = [
        ("n_rows", C.c_uint64), ("n_children", C.c_uint64), ("n_ctl", C.c_uint64),
        ("n_heartbeat", C.c_uint64), ("err_kind", C.c_int32), ("path", C.c_uint32),
        ("err_offset", C.c_uint64),
    ]


# every symbol include/nxg_codec.h declares, with its ctypes signature
SIGNATURES = {
    "nxg_ctx_new": (C.c_void_p, [C.c_int, C.POINTER(NetidxError)]),
    "nxg_ctx_destroy": (None, [C.c_void_p]),
    "nxg_ctx_set_stream": (C.c_bool, [C.c_void_p, C.c_void_p, C.POINTER(NetidxError)]),
    "nxg_ctx_stream": (C.c_void_p, [C.c_void_p]),
    "nxg_error_free": (None, [C.POINTER(NetidxError)]),
    "nxg_version": (C.c_char_p, []),
    "nxg_columns_alloc": (C.c_bool, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64,
                                     C.c_uint32, C.POINTER(NxgColumns), C.POINTER(NetidxError)]),
    "nxg_columns_free": (None, [C.c_void_p, C.POINTER(NxgColumns)]),
    "nxg_decode_updates": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(NxgColumns),
                                      C.c_uint32, C.POINTER(NxgStatus), C.POINTER(NetidxError)]),
    "nxg_decode_updates_async": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_uint64,
                                            C.POINTER(NxgColumns), C.c_uint32,
                                            C.POINTER(NetidxError)]),
    "nxg_ctx_sync": (C.c_bool, [C.c_void_p, C.POINTER(NxgStatus), C.POINTER(NetidxError)]),
    "nxg_decode_frames_async": (C.c_bool, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_uint32, C.POINTER(NetidxError)]),
    "nxg_encoded_len": (C.c_bool, [C.c_void_p, C.POINTER(NxgColumns), C.c_void_p,
                                   C.POINTER(C.c_uint64), C.POINTER(NetidxError)]),
    "nxg_encode_updates": (C.c_bool, [C.c_void_p, C.POINTER(NxgColumns), C.c_void_p, C.c_void_p,
                                      C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(NetidxError)]),
    "nxg_encode_updates_async": (C.c_bool, [C.c_void_p, C.POINTER(NxgColumns), C.c_void_p,
                                            C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                            C.POINTER(NetidxError)]),
    "nxg_encode_frames": (C.c_bool, [C.c_void_p, C.POINTER(NxgColumns), C.c_void_p, C.c_void_p,
                                     C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64,
                                     C.POINTER(C.c_uint64), C.POINTER(NetidxError)]),
    "nxg_write_cols_alloc": (C.c_bool, [C.c_void_p, C.c_uint64, C.c_uint32,
                                        C.POINTER(NxgWriteCols), C.POINTER(NetidxError)]),
    "nxg_write_cols_free": (None, [C.c_void_p, C.POINTER(NxgWriteCols)]),
    "nxg_decode_writes": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(NxgColumns),
                                     C.POINTER(NxgWriteCols), C.POINTER(NxgStatus),
                                     C.POINTER(NetidxError)]),
    "nxg_decode_writes_opts": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_uint64,
                                          C.POINTER(NxgColumns), C.POINTER(NxgWriteCols),
                                          C.POINTER(NxgWriteDecodeOpts), C.POINTER(NxgStatus),
                                          C.POINTER(NetidxError)]),
    "nxg_encoded_writes_len": (C.c_bool, [C.c_void_p, C.POINTER(NxgColumns),
                                          C.POINTER(NxgWriteCols), C.c_void_p,
                                          C.POINTER(C.c_uint64), C.POINTER(NetidxError)]),
    "nxg_encode_writes": (C.c_bool, [C.c_void_p, C.POINTER(NxgColumns), C.POINTER(NxgWriteCols),
                                     C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                     C.POINTER(NetidxError)]),
    "nxg_route_writes": (C.c_bool, [C.c_void_p, C.POINTER(NxgWriteTable), C.c_void_p,
                                    C.POINTER(NxgColumns), C.POINTER(NxgWriteCols), C.c_uint64,
                                    C.c_uint64, C.c_uint64, C.POINTER(NxgWriteRoute),
                                    C.POINTER(NetidxError)]),
    "nxg_path_table_new": (C.c_void_p, [C.c_void_p, C.c_uint64, C.c_uint64,
                                        C.POINTER(NetidxError)]),
    "nxg_path_table_free": (None, [C.c_void_p]),
    "nxg_path_table_len": (C.c_uint64, [C.c_void_p]),
    "nxg_path_table_insert": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                         C.POINTER(NetidxError)]),
    "nxg_path_table_remove": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_uint64, C.POINTER(C.c_uint64),
                                         C.POINTER(NetidxError)]),
    "nxg_path_table_lookup": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_uint64, C.c_void_p,
                                         C.POINTER(NetidxError)]),
    "nxg_path_is_plain": (C.c_bool, [C.c_void_p, C.c_uint64]),
    "nxg_path_hash": (C.c_uint64, [C.c_void_p, C.c_uint64]),
    "nxg_route_subscribes": (C.c_bool, [C.c_void_p, C.POINTER(NxgSubscribeTable), C.c_void_p,
                                        C.POINTER(NxgColumns), C.c_uint64, C.c_uint64,
                                        C.c_void_p, C.POINTER(NxgSubscribeRoute),
                                        C.POINTER(NetidxError)]),
    "nxg_route_replies": (C.c_bool, [C.c_void_p, C.POINTER(NxgReplyTable), C.c_void_p,
                                     C.POINTER(NxgColumns), C.c_uint64, C.c_uint64,
                                     C.POINTER(NxgReplyRoute), C.POINTER(NetidxError)]),
    "nxg_decode_range": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                    C.POINTER(NxgColumns), C.POINTER(NxgRange),
                                    C.POINTER(NetidxError)]),
    "nxg_decode_share": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                    C.POINTER(NxgColumns), C.POINTER(C.c_uint64),
                                    C.POINTER(NxgStatus), C.POINTER(NetidxError)]),
    "nxg_range_link": (C.c_bool, [C.POINTER(NxgRange), C.c_uint32, C.c_uint64, C.c_void_p,
                                  C.POINTER(C.c_uint32), C.POINTER(NetidxError)]),
    "nxg_comm_unique_id": (C.c_bool, [C.c_void_p, C.POINTER(NetidxError)]),
    "nxg_comm_init": (C.c_void_p, [C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                   C.POINTER(NetidxError)]),
    "nxg_comm_init_ops": (C.c_void_p, [C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                       C.POINTER(NetidxError)]),
    "nxg_comm_destroy": (None, [C.c_void_p]),
    "nxg_encode_allgather": (C.c_bool, [C.c_void_p, C.c_void_p, C.POINTER(NxgColumns),
                                        C.c_void_p, C.c_void_p, C.c_uint64,
                                        C.POINTER(C.c_uint64), C.c_void_p,
                                        C.POINTER(NetidxError)]),
    "nxg_decode_sharded": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                      C.POINTER(NxgColumns), C.POINTER(C.c_uint64),
                                      C.POINTER(NxgRange), C.POINTER(NetidxError)]),
    "nxg_partition_by_tag": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(NetidxError)]),
    "nxg_dispatch_updates": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                        C.c_void_p, C.POINTER(NetidxError)]),
    "nxg_publish_commit": (C.c_bool, [C.c_void_p, C.c_void_p, C.POINTER(NxgColumns), C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(NetidxError)]),
    "nxg_publish_unsubscribes": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                            C.c_uint32, C.c_void_p, C.POINTER(NetidxError)]),
    "nxg_record_entries": (C.c_bool, [C.c_void_p, C.POINTER(NxgColumns), C.c_void_p,
                                      C.POINTER(NxgDispatch), C.c_uint32,
                                      C.POINTER(NxgRecordTable), C.POINTER(NxgRecordBatches),
                                      C.POINTER(NetidxError)]),
    "nxg_archive_index_records": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                             C.c_uint32, C.POINTER(NxgRecordTable),
                                             C.POINTER(NxgArchiveIndexes),
                                             C.POINTER(NetidxError)]),
    "nxg_archive_scan_index": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                          C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                          C.c_void_p, C.POINTER(C.c_uint64),
                                          C.POINTER(NetidxError)]),
    "nxg_oneshot_pack_pathmap": (C.c_bool, [C.c_void_p, C.POINTER(NxgOneshotPaths), C.c_void_p,
                                            C.POINTER(NxgOneshotPathmap),
                                            C.POINTER(NetidxError)]),
    "nxg_oneshot_pack_deltas": (C.c_bool, [C.c_void_p, C.POINTER(NxgColumns), C.c_void_p,
                                           C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_uint64, C.POINTER(NxgOneshotDeltas),
                                           C.POINTER(NetidxError)]),
    "nxg_oneshot_shard_layout": (C.c_bool, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                            C.POINTER(NxgOneshotShardLayout),
                                            C.POINTER(NetidxError)]),
    "nxg_oneshot_reply_head": (C.c_bool, [C.c_void_p, C.c_uint64, C.c_void_p,
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                          C.POINTER(NetidxError)]),
    "nxg_oneshot_assemble_shard": (C.c_bool, [C.c_void_p, C.POINTER(NxgOneshotShardLayout),
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                              C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                              C.POINTER(NetidxError)]),
    "nxg_encode_clients": (C.c_bool, [C.c_void_p, C.POINTER(NxgColumns), C.c_void_p,
                                      C.POINTER(NxgDispatch), C.c_uint32,
                                      C.POINTER(NxgClientFrames), C.POINTER(NetidxError)]),
    "nxg_value_table_init": (C.c_bool, [C.c_void_p, C.POINTER(NxgValueTable),
                                        C.POINTER(NetidxError)]),
    "nxg_value_table_apply": (C.c_bool, [C.c_void_p, C.POINTER(NxgValueTable),
                                         C.POINTER(NxgColumns), C.c_void_p, C.c_uint64,
                                         C.c_void_p, C.POINTER(NxgValueApply),
                                         C.POINTER(NetidxError)]),
    "nxg_value_table_rebuild": (C.c_bool, [C.c_void_p, C.POINTER(NxgValueTable),
                                           C.POINTER(NxgColumns), C.c_void_p, C.c_uint64,
                                           C.c_void_p, C.POINTER(NxgValueTable),
                                           C.POINTER(NxgValueApply), C.POINTER(NetidxError)]),
    "nxg_value_table_set_unsubscribed": (C.c_bool, [C.c_void_p, C.POINTER(NxgValueTable),
                                                    C.c_void_p, C.c_uint64,
                                                    C.POINTER(NetidxError)]),
    "nxg_zstd_dict_new": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_uint64,
                                       C.POINTER(NetidxError)]),
    "nxg_zstd_dict_free": (None, [C.c_void_p]),
    "nxg_archive_decompress": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                          C.POINTER(NxgArchiveRecord), C.c_uint32, C.c_bool,
                                          C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                          C.POINTER(NetidxError)]),
    "nxg_archive_compress": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                        C.POINTER(NxgArchiveRecord), C.c_uint32, C.c_bool,
                                        C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                        C.POINTER(NetidxError)]),
    "nxg_archive_compress_opts": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                             C.POINTER(NxgArchiveRecord), C.c_uint32, C.c_bool,
                                             C.POINTER(NxgZstdCompressOpts), C.c_void_p,
                                             C.c_uint64, C.POINTER(C.c_uint64),
                                             C.POINTER(NetidxError)]),
    "nxg_decode_archive_batch": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_uint64,
                                            C.POINTER(NxgColumns), C.POINTER(NxgStatus),
                                            C.POINTER(C.c_uint64), C.POINTER(NetidxError)]),
    "nxg_encode_archive_batch": (C.c_bool, [C.c_void_p, C.POINTER(NxgColumns), C.c_void_p,
                                            C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                            C.POINTER(NetidxError)]),
    "nxg_archive_decode_window": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_uint64,
                                             C.POINTER(NxgArchiveRecord), C.c_uint32,
                                             C.POINTER(NxgArchiveWindowOpts),
                                             C.POINTER(NxgColumns),
                                             C.POINTER(NxgArchiveBatchInfo),
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                             C.POINTER(NetidxError)]),
    "nxg_archive_build_image": (C.c_bool, [C.c_void_p, C.POINTER(NxgColumns), C.c_uint64,
                                           C.c_void_p, C.POINTER(NxgArchiveImage),
                                           C.POINTER(NetidxError)]),
    "nxg_replay_window": (C.c_bool, [C.c_void_p, C.POINTER(NxgColumns),
                                     C.POINTER(NxgArchiveBatchInfo), C.c_uint32,
                                     C.POINTER(NxgReplayTable), C.POINTER(NxgReplayRows),
                                     C.POINTER(NetidxError)]),
    "nxg_replay_image": (C.c_bool, [C.c_void_p, C.POINTER(NxgArchiveImage), C.c_void_p,
                                    C.c_uint64, C.POINTER(NxgReplayTable),
                                    C.POINTER(NxgReplayRows), C.POINTER(NetidxError)]),
    "nxg_session_connect": (C.c_void_p, [C.c_char_p, C.c_uint16, C.POINTER(NetidxError)]),
    "nxg_session_listen": (C.c_void_p, [C.c_char_p, C.c_uint16, C.POINTER(C.c_uint16),
                                        C.POINTER(NetidxError)]),
    "nxg_session_accept": (C.c_void_p, [C.c_void_p, C.POINTER(NetidxError)]),
    "nxg_session_close": (None, [C.c_void_p]),
    "nxg_session_stats": (None, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "nxg_session_send": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(NetidxError)]),
    "nxg_session_recv_frame": (C.c_bool, [C.c_void_p, C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_uint64), C.POINTER(NetidxError)]),
    "nxg_session_recv_decode": (C.c_bool, [C.c_void_p, C.c_void_p, C.POINTER(NxgColumns),
                                           C.c_uint32, C.POINTER(NxgStatus),
                                           C.POINTER(C.c_uint64), C.POINTER(NetidxError)]),
    "nxg_session_publish": (C.c_bool, [C.c_void_p, C.c_void_p, C.POINTER(NxgColumns), C.c_void_p,
                                       C.POINTER(C.c_uint64), C.POINTER(NetidxError)]),
    "nxg_msg_subscribe": (C.c_int64, [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint16, C.c_uint64,
                                      C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p,
                                      C.c_uint64]),
    "nxg_msg_subscribed": (C.c_int64, [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint8, C.c_uint64,
                                       C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]),
    "nxg_msg_heartbeat": (C.c_int64, [C.c_void_p, C.c_uint64]),
    "nxg_msg_update": (C.c_int64, [C.c_uint64, C.c_uint8, C.c_uint64, C.c_uint32, C.c_void_p,
                                   C.c_void_p, C.c_uint64]),
    "nxg_resolver_start": (C.c_void_p, [C.c_char_p, C.c_uint16, C.POINTER(C.c_uint16),
                                        C.c_uint64, C.POINTER(NetidxError)]),
    "nxg_resolver_stop": (None, [C.c_void_p]),
    "nxg_resolver_n_published": (C.c_uint64, [C.c_void_p]),
    "nxg_resolver_connect_write": (C.c_void_p, [C.c_char_p, C.c_uint16, C.c_uint32, C.c_uint16,
                                                C.POINTER(C.c_uint64), C.POINTER(NetidxError)]),
    "nxg_resolver_connect_read": (C.c_void_p, [C.c_char_p, C.c_uint16, C.POINTER(NetidxError)]),
    "nxg_resolver_client_close": (None, [C.c_void_p]),
    "nxg_resolver_publish": (C.c_bool, [C.c_void_p, C.c_char_p, C.c_uint64,
                                        C.POINTER(NetidxError)]),
    "nxg_resolver_resolve": (C.c_bool, [C.c_void_p, C.c_char_p, C.c_uint64,
                                        C.POINTER(NxgResolved), C.POINTER(NetidxError)]),
    "nxg_msg_parse": (C.c_bool, [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(NxgCtlMsg),
                                 C.POINTER(NetidxError)]),
    "nxg_frame_reader_new": (C.c_void_p, [C.POINTER(NetidxError)]),
    "nxg_frame_reader_free": (None, [C.c_void_p]),
    "nxg_frame_reader_push": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_uint64,
                                         C.POINTER(NetidxError)]),
    "nxg_frame_reader_next": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_uint64), C.POINTER(NetidxError)]),
    "nxg_frame_reader_buffered": (C.c_uint64, [C.c_void_p]),
    "nxg_frame_split": (C.c_int64, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    "nxg_frame_header": (None, [C.c_uint32, C.c_bool, C.c_void_p]),
    "nxg_frame_parse_header": (C.c_uint32, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_bool)]),
}

_lib = None


def lib():
    """Load libnxg_codec.so (loud failure if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CodecError(f"{LIB_PATH} missing: build it (python -c 'import __graft_entry__ as g; g.build()')")
        # One HIP runtime per process: torch carries its own libamdhip64 and must load it before
        # this library's NEEDED libamdhip64.so.7 is resolved (the loader then reuses torch's); if
        # /opt/rocm's were loaded first, torch would find no GPU ("No HIP GPUs are available").
        try:
            import torch
            torch.cuda.is_available()
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("NXG_LIB") and not hasattr(L, name):
                continue  # an A/B build of an older source may lack newer entry points
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _check(ok, err):
    if not ok:
        msg = err.msg.decode() if err.msg else "unknown error"
        lib().nxg_error_free(C.byref(err))
        raise CodecError(msg)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class ZstdDict:
    """A device-resident zstd dictionary (nxg_zstd_dict_new / _free)."""

    def __init__(self, h):
        self.h = h

    def close(self):
        if self.h:
            lib().nxg_zstd_dict_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Columns:
    """Columnar batch (include/nxg_codec.h). Arrays are torch tensors on `device` (or pinned
    host numpy-backed tensors when device is 'cpu')."""

    FIELDS = [("id", "torch.int64", "rows"), ("fixed", "torch.int64", "rows"),
              ("tag", "torch.uint8", "rows"), ("aux", "torch.int32", "rows"),
              ("ctag", "torch.uint8", "children"), ("cfixed", "torch.int64", "children"),
              ("caux", "torch.int32", "children"), ("ctl_row", "torch.int64", "ctl"),
              ("ctl_off", "torch.int64", "ctl"), ("ctl_len", "torch.int32", "ctl"),
              ("ctl_variant", "torch.uint8", "ctl")]

    def __init__(self, cap_rows, cap_children=0, cap_ctl=0, layout=LAYOUT_MIXED, device="cuda"):
        import torch
        self.device = torch.device(device)
        self.layout = layout
        self.caps = {"rows": max(cap_rows, 1), "children": max(cap_children, 1),
                     "ctl": max(cap_ctl, 1)}
        self.t = {}
        dt = {"torch.int64": torch.int64, "torch.int32": torch.int32, "torch.uint8": torch.uint8}
        for name, d, kind in self.FIELDS:
            if layout == LAYOUT_F64 and name not in ("id", "fixed"):
                self.t[name] = None
                continue
            x = torch.zeros(self.caps[kind], dtype=dt[d], device=self.device)
            if self.device.type == "cpu":
                x = x.pin_memory()
            self.t[name] = x
        self.s = NxgColumns()
        self.s.layout = layout
        self.s.mem = MEM_DEVICE if self.device.type == "cuda" else MEM_HOST
        self.s.cap_rows, self.s.cap_children, self.s.cap_ctl = (
            self.caps["rows"], self.caps["children"], self.caps["ctl"])
        for name, _, _ in self.FIELDS:
            setattr(self.s, name, _ptr(self.t[name]).value)
        if self.device.type == "cuda":
            # the zero fill ran on torch's current stream; a codec on another stream (set_stream)
            # must not start writing before it is done
            torch.cuda.synchronize(self.device)

    @classmethod
    def for_frame(cls, nbytes, layout=LAYOUT_MIXED, device="cuda"):
        """Capacity bounds of include/nxg_codec.h for a frame of `nbytes`."""
        return cls(nbytes // 4 + 1, nbytes + 1, nbytes // 2 + 1, layout, device)

    def __getattr__(self, k):
        t = self.__dict__.get("t", {})
        if k in t:
            return t[k]
        raise AttributeError(k)

    @property
    def n_rows(self):
        return self.s.n_rows

    def numpy(self):
        """Trimmed host copy: {field: ndarray} (unsigned views)."""
        n = {"rows": self.s.n_rows, "children": self.s.n_children, "ctl": self.s.n_ctl}
        out = {}
        u = {"torch.int64": np.uint64, "torch.int32": np.uint32, "torch.uint8": np.uint8}
        for name, d, kind in self.FIELDS:
            x = self.t[name]
            if x is None:
                continue
            out[name] = x[: n[kind]].cpu().numpy().view(u[d])
        if self.s.layout == LAYOUT_F64:  # homogeneous result: tag 9 implied, aux unused
            out["tag"] = np.full(n["rows"], 9, np.uint8)
            if "aux" in out:
                out["aux"] = np.zeros(n["rows"], np.uint32)
        out["n_heartbeat"] = self.s.n_heartbeat
        out["layout"] = self.s.layout
        return out


class WindowCapacity(CodecError):
    """nxg_archive_decode_window: the columns are too small; need_rows / need_children are the
    exact totals."""

    def __init__(self, msg, need_rows, need_children):
        super().__init__(msg)
        self.need_rows, self.need_children = need_rows, need_children


class ArchiveImage:
    """The image of a decoded window (nxg_archive_build_image): id / tag / fixed / aux / src_row
    tensors of n_rows winners in ascending Id order, n_filtered rows dropped by `keep`. It
    borrows the window: children and text stay where the window decode put them."""

    def __init__(self, cap, device):
        import torch
        n = max(cap, 1)
        self.id = torch.zeros(n, dtype=torch.int64, device=device)
        self.tag = torch.zeros(n, dtype=torch.uint8, device=device)
        self.fixed = torch.zeros(n, dtype=torch.int64, device=device)
        self.aux = torch.zeros(n, dtype=torch.int32, device=device)
        self.src_row = torch.zeros(n, dtype=torch.int64, device=device)
        torch.cuda.synchronize(device)  # (as Columns: the zero fill is done)
        self.s = NxgArchiveImage()
        self.s.cap_rows = n
        for k in ("id", "tag", "fixed", "aux", "src_row"):
            setattr(self.s, k, getattr(self, k).data_ptr())

    @property
    def n_rows(self):
        return self.s.n_rows

    @property
    def n_filtered(self):
        return self.s.n_filtered

    def numpy(self):
        n = self.s.n_rows
        return {"id": self.id[:n].cpu().numpy().view(np.uint64), "tag": self.tag[:n].cpu().numpy(),
                "fixed": self.fixed[:n].cpu().numpy().view(np.uint64),
                "aux": self.aux[:n].cpu().numpy().view(np.uint32),
                "src_row": self.src_row[:n].cpu().numpy().view(np.uint64)}

    def columns(self, window_cols):
        """The image as columns for encode_archive(view, heap=the window's buffer): the image's
        row arrays with the window's child arrays (a view; both must stay alive)."""
        v = _ColumnsView()
        v.keep = (self, window_cols)
        v.id, v.tag, v.fixed, v.aux = self.id, self.tag, self.fixed, self.aux
        v.s = NxgColumns()
        C.memmove(C.byref(v.s), C.byref(window_cols.s), C.sizeof(NxgColumns))
        v.s.cap_rows, v.s.n_rows = self.s.cap_rows, self.s.n_rows
        v.s.n_ctl = 0
        for k in ("id", "tag", "fixed", "aux"):
            setattr(v.s, k, getattr(self, k).data_ptr())
        return v


class _ColumnsView:
    pass


class ReplayRows:
    """The update rows of a replayed window or image (nxg_replay_window / nxg_replay_image): id /
    tag / fixed / aux / src_row tensors of n_rows rows, rec_off (n_recs + 1 entries: record i's
    updates are rows [rec_off[i], rec_off[i+1])) and miss_row (cap_miss entries). n_done, n_dropped
    and n_miss as the call wrote them. The rows borrow the window: children and text stay where the
    window decode put them. `arrays`: caller-made tensors to write into instead (any of the seven
    names; cap_rows / cap_miss then state what the call may write)."""

    ROW_ARRAYS = (("id", "int64"), ("tag", "uint8"), ("fixed", "int64"), ("aux", "int32"),
                  ("src_row", "int64"))

    def __init__(self, cap_rows, n_recs, cap_miss=0, device="cuda", arrays=None):
        import torch
        arrays = arrays or {}
        for k, dt in self.ROW_ARRAYS:
            setattr(self, k, arrays[k] if k in arrays else torch.zeros(
                max(cap_rows, 1), dtype=getattr(torch, dt), device=device))
        self.rec_off = arrays["rec_off"] if "rec_off" in arrays else torch.zeros(
            n_recs + 1, dtype=torch.int64, device=device)
        self.miss_row = arrays["miss_row"] if "miss_row" in arrays else torch.zeros(
            max(cap_miss, 1), dtype=torch.int64, device=device)
        torch.cuda.synchronize(device)  # (as Columns: the zero fill is done)
        self.n_recs = n_recs
        self.s = NxgReplayRows()
        self.s.cap_rows, self.s.cap_miss = cap_rows, cap_miss
        for k in ("id", "tag", "fixed", "aux", "src_row", "rec_off", "miss_row"):
            setattr(self.s, k, getattr(self, k).data_ptr())
        self._off = None

    n_rows = property(lambda self: self.s.n_rows)
    n_dropped = property(lambda self: self.s.n_dropped)
    n_done = property(lambda self: self.s.n_done)
    n_miss = property(lambda self: self.s.n_miss)

    def offsets(self):
        """rec_off on the host (uint64), read once per call."""
        if self._off is None:
            self._off = self.rec_off[:self.n_recs + 1].cpu().numpy().view(np.uint64)
        return self._off

    def misses(self):
        """The listed miss rows on the host (uint64): min(n_miss, cap_miss) of them."""
        n = min(self.s.n_miss, self.s.cap_miss)
        return self.miss_row[:n].cpu().numpy().view(np.uint64)

    def numpy(self):
        n = self.s.n_rows
        u = {"int64": np.uint64, "uint8": np.uint8, "int32": np.uint32}
        return {k: getattr(self, k)[:n].cpu().numpy().view(u[dt]) for k, dt in self.ROW_ARRAYS}

    def _view(self, window_cols, lo, hi):
        v = _ColumnsView()
        v.keep = (self, window_cols)
        v.s = NxgColumns()
        C.memmove(C.byref(v.s), C.byref(window_cols.s), C.sizeof(NxgColumns))
        v.s.cap_rows = v.s.n_rows = hi - lo
        v.s.n_ctl = 0
        for k in ("id", "tag", "fixed", "aux"):
            t = getattr(self, k)[lo:hi]
            setattr(v, k, t)
            setattr(v.s, k, t.data_ptr() if hi > lo else getattr(self, k).data_ptr())
        v.src_row = self.src_row[lo:hi]
        return v

    def columns(self, window_cols):
        """Rows [0, n_rows) as the Columns view publish_commit, encode_clients and
        ValueTable.apply take (heap = the window's buffer): the row arrays with the window's child
        arrays (a view; both must stay alive)."""
        return self._view(window_cols, 0, int(self.s.n_rows))

    def record(self, i, window_cols):
        """Record i's updates as such a view (Speed::Limited: one commit per record): the same
        arrays at offset rec_off[i]."""
        off = self.offsets()
        return self._view(window_cols, int(off[i]), int(off[i + 1]))


class WriteCols:
    """The two further fields of To::Write rows (NxgWriteCols): wflags (WRITE_REPLY |
    WRITE_NO_WID) and wid (the WriteId) per row. torch tensors on `device` (pinned host memory
    for 'cpu'), beside a Columns of at most cap_rows rows."""

    def __init__(self, cap_rows, device="cuda"):
        import torch
        self.device = torch.device(device)
        n = max(cap_rows, 1)
        self.wflags = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self.wid = torch.zeros(n, dtype=torch.int64, device=self.device)
        if self.device.type == "cpu":
            self.wflags, self.wid = self.wflags.pin_memory(), self.wid.pin_memory()
        self.s = NxgWriteCols()
        self.s.mem = MEM_DEVICE if self.device.type == "cuda" else MEM_HOST
        self.s.cap_rows = n
        self.s.wflags, self.s.wid = self.wflags.data_ptr(), self.wid.data_ptr()
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)  # (as Columns: the zero fill is done)

    def numpy(self, n_rows):
        """Host copy of the first n_rows rows: {"wflags": u8, "wid": u64}."""
        return {"wflags": self.wflags[:n_rows].cpu().numpy(),
                "wid": self.wid[:n_rows].cpu().numpy().view(np.uint64)}


def _frame_ptr(frame):
    """(pointer, keep-alive) of a frame given as bytes, ndarray, tensor or device pointer."""
    if isinstance(frame, (bytes, bytearray, memoryview)):
        keep = np.frombuffer(bytes(frame), np.uint8)
        return keep.ctypes.data, keep
    if isinstance(frame, np.ndarray):
        keep = np.ascontiguousarray(frame)
        return keep.ctypes.data, keep
    if hasattr(frame, "data_ptr"):
        return frame.data_ptr(), frame
    return int(frame), None


class Codec:
    """One codec context per connection/thread (NxgCtx)."""

    def __init__(self, device=0):
        err = NetidxError()
        self.ctx = lib().nxg_ctx_new(device, C.byref(err))
        _check(self.ctx is not None, err)
        self.device = device

    def close(self):
        if self.ctx:
            lib().nxg_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        err = NetidxError()
        _check(lib().nxg_ctx_set_stream(self.ctx, C.c_void_p(stream_ptr), C.byref(err)), err)

    def decode_into(self, frame, nbytes, cols, flags=0, check=True):
        """frame: device pointer (int), torch tensor or bytes. Returns NxgStatus."""
        keep = None
        if isinstance(frame, (bytes, bytearray, memoryview)):
            keep = np.frombuffer(bytes(frame), np.uint8)
            ptr = keep.ctypes.data
        elif isinstance(frame, np.ndarray):
            keep = np.ascontiguousarray(frame)
            ptr = keep.ctypes.data
        elif hasattr(frame, "data_ptr"):
            ptr = frame.data_ptr()
        else:
            ptr = int(frame)
        st, err = NxgStatus(), NetidxError()
        ok = lib().nxg_decode_updates(self.ctx, C.c_void_p(ptr), nbytes, C.byref(cols.s), flags,
                                      C.byref(st), C.byref(err))
        _check(ok, err)
        if check and st.err_kind:
            raise PackError(st.err_kind, st.err_offset)
        return st

    def decode_archive(self, buf, nbytes, cols, check=True):
        """An archive batch (Vec<BatchItem>, netidx-archive logfile/mod.rs:150-205) in device
        memory into MIXED device columns. Returns (NxgStatus, bytes consumed)."""
        ptr = buf.data_ptr() if hasattr(buf, "data_ptr") else int(buf)
        st, err, used = NxgStatus(), NetidxError(), C.c_uint64(0)
        _check(lib().nxg_decode_archive_batch(self.ctx, C.c_void_p(ptr), nbytes, C.byref(cols.s),
                                              C.byref(st), C.byref(used), C.byref(err)), err)
        if check and st.err_kind:
            raise PackError(st.err_kind, st.err_offset)
        return st, used.value

    def encode_archive(self, cols, heap=None, out=None):
        """Device MIXED columns -> an archive batch (Vec<BatchItem>). Returns a uint8 tensor on
        the device (out=None), or the length written into `out` (a device tensor)."""
        import torch
        err, n = NetidxError(), C.c_uint64(0)
        if out is None:
            _check(lib().nxg_encode_archive_batch(self.ctx, C.byref(cols.s), _heap_ptr(heap),
                                                  None, 0, C.byref(n), C.byref(err)), err)
            out = torch.empty(max(n.value, 1), dtype=torch.uint8, device=cols.id.device)
            _check(lib().nxg_encode_archive_batch(self.ctx, C.byref(cols.s), _heap_ptr(heap),
                                                  C.c_void_p(out.data_ptr()), out.numel(),
                                                  C.byref(n), C.byref(err)), err)
            return out[: n.value]
        _check(lib().nxg_encode_archive_batch(self.ctx, C.byref(cols.s), _heap_ptr(heap),
                                              C.c_void_p(out.data_ptr()), out.numel(), C.byref(n),
                                              C.byref(err)), err)
        return n.value

    def zstd_dict(self, data):
        """A compressed archive's zstd dictionary on the device (nxg_zstd_dict_new)."""
        b = bytes(data)
        a = (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b + b"\0")
        err = NetidxError()
        h = lib().nxg_zstd_dict_new(self.ctx, a, len(b), C.byref(err))
        _check(bool(h), err)
        return ZstdDict(h)

    def archive_decompress(self, src, records, indexed=False, zdict=None, out=None):
        """Compressed archive records (host bytes `src`, [(off, len)] after each RecordHeader)
        decompressed on the device (nxg_archive_decompress). Returns (device uint8 tensor,
        [(out_off, out_len, err)])."""
        import torch
        b = src if isinstance(src, np.ndarray) else np.frombuffer(bytes(src), np.uint8)
        b = np.ascontiguousarray(b)
        n = len(records)
        recs = (NxgArchiveRecord * max(n, 1))()
        for i, (o, ln) in enumerate(records):
            recs[i].off, recs[i].len = o, ln
        need, err = C.c_uint64(0), NetidxError()
        dh = zdict.h if zdict else None
        _check(lib().nxg_archive_decompress(self.ctx, dh, C.c_void_p(b.ctypes.data), len(b), recs,
                                            n, indexed, None, 0, C.byref(need), C.byref(err)), err)
        if out is None:
            out = torch.empty(max(need.value, 1), dtype=torch.uint8, device="cuda")
        _check(lib().nxg_archive_decompress(self.ctx, dh, C.c_void_p(b.ctypes.data), len(b), recs,
                                            n, indexed, C.c_void_p(out.data_ptr()), out.numel(),
                                            C.byref(need), C.byref(err)), err)
        return out, [(recs[i].out_off, recs[i].out_len, recs[i].err) for i in range(n)]

    def archive_decode_window(self, buf, recs, cols, big_record_bytes=0):
        """A window of archive records decoded in one call (nxg_archive_decode_window). buf: the
        device uint8 tensor holding the batches; recs: [(out_off, out_len)] or [(out_off, out_len,
        err)] (archive_decompress's list feeds straight in); cols: MIXED device Columns. Returns
        the per-record infos (NxgArchiveBatchInfo). Raises WindowCapacity when cols is too
        small."""
        n = len(recs)
        r = (NxgArchiveRecord * max(n, 1))()
        for i, t in enumerate(recs):
            r[i].out_off, r[i].out_len = t[0], t[1]
            r[i].err = t[2] if len(t) > 2 else 0
        info = (NxgArchiveBatchInfo * max(n, 1))()
        opts = NxgArchiveWindowOpts(big_record_bytes)
        nr, nc, err = C.c_uint64(0), C.c_uint64(0), NetidxError()
        ok = lib().nxg_archive_decode_window(self.ctx, C.c_void_p(buf.data_ptr()), buf.numel(), r,
                                             n, C.byref(opts), C.byref(cols.s), info,
                                             C.byref(nr), C.byref(nc), C.byref(err))
        if not ok and (nr.value > cols.s.cap_rows or nc.value > cols.s.cap_children):
            msg = err.msg.decode() if err.msg else "capacity"
            lib().nxg_error_free(C.byref(err))
            raise WindowCapacity(msg, nr.value, nc.value)
        _check(ok, err)
        return [info[i] for i in range(n)]

    def archive_build_image(self, cols, n_ids, keep=None):
        """The image of a decoded window (nxg_archive_build_image): the last row per Id, rows
        whose Id has keep[id] == 0 dropped (keep: a device uint8 tensor of n_ids entries, or
        None). Returns an ArchiveImage; .columns(cols) is the view encode_archive takes."""
        img = ArchiveImage(min(n_ids, cols.s.n_rows), cols.id.device)
        err = NetidxError()
        _check(lib().nxg_archive_build_image(self.ctx, C.byref(cols.s), n_ids, _ptr(keep),
                                             C.byref(img.s), C.byref(err)), err)
        return img

    @staticmethod
    def _replay_finish(ok, err, out):
        out._off = None
        if not ok:
            msg = err.msg.decode() if err.msg else "unknown error"
            lib().nxg_error_free(C.byref(err))
            e = CodecError(msg)
            e.rows = out  # (a capacity short: n_rows holds the need)
            raise e
        return out

    def replay_window(self, cols, infos, table, out=None, cap_miss=64):
        """A decoded window as publisher update rows (nxg_replay_window; process_batch,
        session_shard.rs:196-245). cols / infos: archive_decode_window's columns and per-record
        infos (or (row_off, n_rows) pairs; a tail infos[k:] replays from record k); table: the
        device int64 tensor pub_id_of_arch (the publisher Id, REPLAY_DROP or REPLAY_MISS per
        archive Id). Returns a ReplayRows (`out`, or a new one of the window's rows): stopped in
        front of record n_done < len(infos) when that record holds Ids to publish first (misses()).
        A CodecError raised here carries the ReplayRows as `.rows`."""
        n = len(infos)
        info = (NxgArchiveBatchInfo * max(n, 1))()
        for i, t in enumerate(infos):
            if isinstance(t, NxgArchiveBatchInfo):
                info[i].row_off, info[i].n_rows = t.row_off, t.n_rows
            else:
                info[i].row_off, info[i].n_rows = t[0], t[1]
        if out is None:
            out = ReplayRows(int(cols.s.n_rows), n, cap_miss, cols.id.device)
        tab = NxgReplayTable(table.numel(), table.data_ptr() if table.numel() else None)
        err = NetidxError()
        ok = lib().nxg_replay_window(self.ctx, C.byref(cols.s), info, n, C.byref(tab),
                                     C.byref(out.s), C.byref(err))
        return self._replay_finish(ok, err, out)

    def replay_image(self, image, order, table, out=None, cap_miss=64):
        """reimage (session_shard.rs:375-409) as publisher update rows (nxg_replay_image): image:
        archive_build_image's; order: the pathmap's archive Ids, a device int32 tensor (uint32
        storage); table as for replay_window. Returns a ReplayRows of one record; misses() lists
        the positions of `order` whose Ids are to be published first (they do not stop the call)."""
        n = order.numel()
        if out is None:
            out = ReplayRows(n, 1, cap_miss, order.device)
        tab = NxgReplayTable(table.numel(), table.data_ptr() if table.numel() else None)
        err = NetidxError()
        ok = lib().nxg_replay_image(self.ctx, C.byref(image.s),
                                    C.c_void_p(order.data_ptr() if n else None), n,
                                    C.byref(tab), C.byref(out.s), C.byref(err))
        return self._replay_finish(ok, err, out)

    def archive_compress(self, src, records, indexed=False, zdict=None, literals=0):
        """Uncompressed archive records (host bytes `src`, [(off, len)] after each RecordHeader)
        compressed on the device (nxg_archive_compress_opts). Returns (host uint8 array,
        [(out_off, out_len, err)]): record i's compressed record -- u32 BE length | index | zstd
        frame -- is out[out_off:out_off + out_len]. literals: ZSTD_LIT_DICT_TREE (0, Huffman
        literals with the dictionary's tree only) or ZSTD_LIT_BLOCK_TREES (1, a block may build and
        describe its own tree)."""
        b = src if isinstance(src, np.ndarray) else np.frombuffer(bytes(src), np.uint8)
        b = np.ascontiguousarray(b)
        n = len(records)
        recs = (NxgArchiveRecord * max(n, 1))()
        for i, (o, ln) in enumerate(records):
            recs[i].off, recs[i].len = o, ln
        need, err = C.c_uint64(0), NetidxError()
        dh = zdict.h if zdict else None
        opts = NxgZstdCompressOpts(literals=literals)
        f = lib().nxg_archive_compress_opts
        _check(f(self.ctx, dh, C.c_void_p(b.ctypes.data), len(b), recs, n, indexed,
                 C.byref(opts), None, 0, C.byref(need), C.byref(err)), err)
        out = np.zeros(max(need.value, 1), np.uint8)
        _check(f(self.ctx, dh, C.c_void_p(b.ctypes.data), len(b), recs, n, indexed,
                 C.byref(opts), C.c_void_p(out.ctypes.data), need.value, C.byref(need),
                 C.byref(err)), err)
        return out, [(recs[i].out_off, recs[i].out_len, recs[i].err) for i in range(n)]

    def decode_batch(self, frame, layout=LAYOUT_MIXED, flags=0, device="cuda"):
        """Decode one frame payload; returns (Columns, NxgStatus)."""
        n = len(frame) if not hasattr(frame, "numel") else frame.numel()
        cols = Columns.for_frame(n, layout, device)
        st = self.decode_into(frame, n, cols, flags)
        return cols, st

    def last_status(self):
        """(fast_fail, irregular, path, n_rows, err_kind, timeout) of the last completed decode's
        device status (diagnostics, not ABI)."""
        a = (C.c_ulonglong * 6)()
        lib().nxg_debug_status(C.c_void_p(self.ctx), a)
        return list(a)

    def last_diag(self):
        """DevStatus.diag of the last completed decode (diagnostics, not ABI): for an f64 frame,
        diag[1] == 1 when the sequential-id decoder (nxg_decode_f64_seq.hip) produced it."""
        a = (C.c_ulonglong * 8)()
        lib().nxg_debug_diag(C.c_void_p(self.ctx), a)
        return list(a)

    def last_route(self):
        """(decoder, seq_left, irregular_left, mix_left) (diagnostics, not ABI): the decoder that
        produced the last completed decode -- 1 length-run, 2 single-pass, 3 fast mixed,
        4 sequential-id, 0 general -- and the context's three countdowns."""
        a = (C.c_uint * 4)()
        lib().nxg_debug_route(C.c_void_p(self.ctx), a)
        return tuple(a)

    def last_encode_kernel(self):
        """Which f64 encoder wrote the last f64 encode (diagnostics, not ABI): "seq" for the
        sequential-id kernel (nxg_encode_f64_seq.hip), "tile" for the tiled look-back kernel."""
        f = lib().nxg_debug_enc_kernel
        f.restype = C.c_uint
        return {1: "seq", 2: "tile"}.get(f(C.c_void_p(self.ctx)), None)

    def decode_async(self, dframe_ptr, nbytes, cols, flags=0):
        err = NetidxError()
        _check(lib().nxg_decode_updates_async(self.ctx, C.c_void_p(dframe_ptr), nbytes,
                                              C.byref(cols.s), flags, C.byref(err)), err)

    def decode_frames_async(self, dframe_ptrs, lens, cols_list, flags=0):
        """A backlog of device frames (nxg_decode_frames_async), decoded in order; frame j into
        cols_list[j] (one Columns object may repeat). Complete with sync()."""
        n = len(dframe_ptrs)
        fp = (C.c_void_p * n)(*[int(p) for p in dframe_ptrs])
        ln = (C.c_uint64 * n)(*[int(x) for x in lens])
        cp = (C.c_void_p * n)(*[C.addressof(c.s) for c in cols_list])
        err = NetidxError()
        _check(lib().nxg_decode_frames_async(self.ctx, n, fp, ln, cp, flags, C.byref(err)), err)

    def sync(self, check=True):
        st, err = NxgStatus(), NetidxError()
        ok = lib().nxg_ctx_sync(self.ctx, C.byref(st), C.byref(err))
        self.__dict__["_pending_len"] = []
        _check(ok, err)
        if check and st.err_kind:
            raise PackError(st.err_kind, st.err_offset)
        return st

    def dispatch_updates(self, table, ids, n_rows=None, cap=None):
        """process_updates_batch (connection.rs:546-567) for decoded rows: `ids` is the device id
        column (int64/uint64 tensor). Returns a Dispatch."""
        import torch
        n = ids.numel() if n_rows is None else int(n_rows)
        dev = ids.device
        streams = table.stream_chan.numel()
        if cap is None:  # each row reaches at most the largest fan-out of any subscription
            offs = table.slot_stream_off.cpu().numpy().view(np.uint32).astype(np.int64)
            cap = n * int((offs[1:] - offs[:-1]).max()) if streams else 0
        chan_off = torch.zeros(table.n_chans + 1, dtype=torch.int64, device=dev)
        ent_sub = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        ent_row = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        last_row = torch.empty(max(table.slot_sub_id.numel(), 1), dtype=torch.int64, device=dev)
        tb = table.c_struct()
        out = NxgDispatch(cap, chan_off.data_ptr(), ent_sub.data_ptr(), ent_row.data_ptr(),
                          last_row.data_ptr(), 0, 0)
        err = NetidxError()
        _check(lib().nxg_dispatch_updates(self.ctx, C.byref(tb), C.c_void_p(ids.data_ptr()), n,
                                          C.byref(out), C.byref(err)), err)
        return Dispatch(chan_off, ent_sub, ent_row, last_row[: table.slot_sub_id.numel()],
                        out.n_entries, out.n_unmatched)

    def partition_by_tag(self, cols, view=None):
        """nxg_partition_by_tag: the type-partitioned view of decoded mixed device columns
        (per-tag dense runs of fixed / aux, the dense index -> row map, the row -> rank map).
        Returns a TagView (its device tensors are reused when `view` is passed)."""
        n = int(cols.s.n_rows)
        if view is None or view.cap < n:
            view = TagView(max(n, 1), cols.device)
        v = NxgTagView()
        v.cap_rows = view.cap
        v.rank, v.row_of = view.rank.data_ptr(), view.row_of.data_ptr()
        v.fixed, v.aux = view.fixed.data_ptr(), view.aux.data_ptr()
        err = NetidxError()
        _check(lib().nxg_partition_by_tag(self.ctx, C.byref(cols.s), C.byref(v), C.byref(err)),
               err)
        view.n_rows = int(v.n_rows)
        view.count = np.frombuffer(bytes(v.count), np.uint64).copy()
        view.off = np.frombuffer(bytes(v.off), np.uint64).copy()
        return view

    def publish_commit(self, table, batch, kind, to_client=None, heap=None, cap=None):
        """UpdateBatch::commit on device columns: `batch` (Columns: id, tag, fixed, aux and the
        children of its Array/Map/Error(Value) values), per-row
        `kind` (PUB_UPDATE / PUB_UPDATE_CHANGED / PUB_UPDATE_CLIENT, uint8 tensor) and
        `to_client` (int32 tensor, for PUB_UPDATE_CLIENT rows). Returns a Dispatch whose
        channels are the clients and whose entries are (Id, row); last_row[slot] = 1 + the row
        that became current."""
        import torch
        n = batch.s.n_rows
        dev = batch.id.device
        if to_client is None:
            to_client = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        if cap is None:
            offs = table.slot_client_off.cpu().numpy().view(np.uint32).astype(np.int64)
            cap = n * max(1, int((offs[1:] - offs[:-1]).max()) if len(offs) > 1 else 1)
        chan_off = torch.zeros(table.n_clients + 1, dtype=torch.int64, device=dev)
        ent_id = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        ent_row = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        n_slots = table.slot_client_off.numel() - 1
        last_row = torch.empty(max(n_slots, 1), dtype=torch.int64, device=dev)
        out = NxgDispatch(cap, chan_off.data_ptr(), ent_id.data_ptr(), ent_row.data_ptr(),
                          last_row.data_ptr(), 0, 0)
        tb = table.c_struct()
        err = NetidxError()
        _check(lib().nxg_publish_commit(self.ctx, C.byref(tb), C.byref(batch.s), _heap_ptr(heap),
                                        C.c_void_p(kind.data_ptr()),
                                        C.c_void_p(to_client.data_ptr()), C.byref(out),
                                        C.byref(err)), err)
        return Dispatch(chan_off, ent_id, ent_row, last_row[:n_slots], out.n_entries,
                        out.n_unmatched)

    def publish_unsubscribes(self, ids, clients, n_clients):
        """The commit's unsubscribes (publisher/mod.rs:820-832): device tensors of Ids (int64)
        and clients (int32), in queue order. Returns a Dispatch whose channels are the clients
        and whose entries are (Id, index in the queue)."""
        import torch
        n = ids.numel()
        dev = ids.device
        chan_off = torch.zeros(n_clients + 1, dtype=torch.int64, device=dev)
        ent_id = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        ent_row = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        out = NxgDispatch(n, chan_off.data_ptr(), ent_id.data_ptr(), ent_row.data_ptr(), None,
                          0, 0)
        err = NetidxError()
        _check(lib().nxg_publish_unsubscribes(self.ctx, C.c_void_p(ids.data_ptr()),
                                              C.c_void_p(clients.data_ptr()), n, n_clients,
                                              C.byref(out), C.byref(err)), err)
        return Dispatch(chan_off, ent_id, ent_row, chan_off[:0], out.n_entries, 0)

    def encode_clients_into(self, batch, dispatch, heap, out_ptr, cap, client_off=None):
        """nxg_encode_clients into device memory at `out_ptr` (0 / None: size only). `dispatch`:
        a Dispatch (publish_commit's, or any chan_off / ent_row device tensors with n_entries).
        Returns (n_bytes, client_off); a CodecError raised here carries n_bytes (what a buffer
        too small would have needed) and client_off."""
        import torch
        n_clients = dispatch.chan_off.numel() - 1
        if client_off is None:
            client_off = torch.empty(n_clients + 1, dtype=torch.int64, device=batch.id.device)
        d = NxgDispatch(dispatch.ent_row.numel(), dispatch.chan_off.data_ptr(),
                        dispatch.ent_sub.data_ptr() if dispatch.ent_sub is not None else None,
                        dispatch.ent_row.data_ptr(), None, int(dispatch.n_entries), 0)
        o = NxgClientFrames(cap, out_ptr or None, client_off.data_ptr(), 0)
        err = NetidxError()
        try:
            _check(lib().nxg_encode_clients(self.ctx, C.byref(batch.s), _heap_ptr(heap),
                                            C.byref(d), n_clients, C.byref(o), C.byref(err)), err)
        except CodecError as e:
            e.n_bytes, e.client_off = int(o.n_bytes), client_off
            raise
        return int(o.n_bytes), client_off

    def encoded_clients_len(self, batch, dispatch, heap=None):
        """The size-only form of encode_clients: (n_bytes, client_off), nothing encoded."""
        return self.encode_clients_into(batch, dispatch, heap, None, 0)

    def encode_clients(self, batch, dispatch, heap=None, out=None):
        """The commit's per-client batches in one call (handle_updates -> queue_send per client):
        `batch` and `heap` as given to publish_commit, `dispatch` its result. Returns (bytes,
        client_off): client c's frame payload is bytes[client_off[c]:client_off[c+1]] (uint8 /
        int64 tensors on the batch's device). `out`: a uint8 device tensor to encode into (all of
        it is the capacity); without one the call sizes first and allocates."""
        import torch
        off = None
        if out is None:
            n, off = self.encoded_clients_len(batch, dispatch, heap)
            out = torch.empty(max(n, 16), dtype=torch.uint8, device=batch.id.device)
            cap = n
        else:
            cap = out.numel()
        n, off = self.encode_clients_into(batch, dispatch, heap, out.data_ptr(), cap, off)
        return out[:n], off

    def record_entries_into(self, batch, dispatch, table, heap, out_ptr, cap, rec_off=None,
                            rec_items=None):
        """nxg_record_entries into device memory at `out_ptr` (0 / None: size only). `dispatch`: a
        Dispatch (dispatch_updates', route_replies' disp, or any chan_off / ent_sub / ent_row
        device tensors with n_entries); `table`: arch_id_of_sub, a uint32 (int32 storage) device
        tensor. Returns (n_bytes, rec_off, rec_items, n_items, n_dropped); a CodecError raised here
        carries n_bytes, rec_off and rec_items."""
        import torch
        n_chans = dispatch.chan_off.numel() - 1
        dev = dispatch.chan_off.device
        if rec_off is None:
            rec_off = torch.empty(n_chans + 1, dtype=torch.int64, device=dev)
        if rec_items is None:
            rec_items = torch.empty(max(n_chans, 1), dtype=torch.int64, device=dev)
        d = NxgDispatch(dispatch.ent_row.numel(), dispatch.chan_off.data_ptr(),
                        dispatch.ent_sub.data_ptr(), dispatch.ent_row.data_ptr(), None,
                        int(dispatch.n_entries), 0)
        t = NxgRecordTable(table.numel(), table.data_ptr() if table.numel() else None)
        o = NxgRecordBatches(cap, out_ptr or None, rec_off.data_ptr(), rec_items.data_ptr(),
                             0, 0, 0)
        err = NetidxError()
        try:
            _check(lib().nxg_record_entries(self.ctx, C.byref(batch.s), _heap_ptr(heap),
                                            C.byref(d), n_chans, C.byref(t), C.byref(o),
                                            C.byref(err)), err)
        except CodecError as e:
            e.n_bytes, e.rec_off, e.rec_items = int(o.n_bytes), rec_off, rec_items
            raise
        return int(o.n_bytes), rec_off, rec_items[:n_chans], int(o.n_items), int(o.n_dropped)

    def recorded_len(self, batch, dispatch, table, heap=None):
        """The size-only form of record_entries: (n_bytes, rec_off, rec_items, n_dropped), nothing
        encoded."""
        n, off, items, _, dropped = self.record_entries_into(batch, dispatch, table, heap, None, 0)
        return n, off, items, dropped

    def record_entries(self, batch, dispatch, table, heap=None, out=None):
        """A dispatch's entries as archive batch records in one call (the recorder's batch loop,
        record.rs:307-347): `batch` and `heap` are what the dispatch was made from, `table`
        arch_id_of_sub (SubId -> archive Id, NO_SLOT: not recorded). Returns (bytes, rec_off,
        rec_items, n_dropped): channel c's record is bytes[rec_off[c]:rec_off[c+1]], rec_items[c]
        items (uint8 / int64 tensors on the dispatch's device). `out`: a uint8 device tensor to
        encode into (all of it is the capacity); without one the call sizes first and allocates."""
        import torch
        off = items = None
        if out is None:
            n, off, items, _ = self.recorded_len(batch, dispatch, table, heap)
            out = torch.empty(max(n, 16), dtype=torch.uint8, device=dispatch.chan_off.device)
            cap = n
        else:
            cap = out.numel()
        n, off, items, _, dropped = self.record_entries_into(batch, dispatch, table, heap,
                                                             out.data_ptr(), cap, off, items)
        return out[:n], off, items, dropped

    def index_records_into(self, key, seg_off, table, out_ptr, cap, idx_off=None, idx_ids=None,
                           n_keys=None):
        """nxg_archive_index_records into device memory at `out_ptr` (0 / None: size only): the
        RecordIndex of every record of `seg_off` (int64 device tensor, n_recs + 1 entries) over
        `key` (int64 device tensor; n_keys: how many of its positions there are, default all).
        `table`: None (key holds archive Ids) or arch_id_of_sub, a uint32 (int32 storage) device
        tensor (key holds SubIds). Returns (n_bytes, idx_off, idx_ids, n_ids_total); a CodecError
        raised here carries n_bytes, idx_off and idx_ids."""
        import torch
        n_recs = seg_off.numel() - 1
        dev = seg_off.device
        if idx_off is None:
            idx_off = torch.empty(n_recs + 1, dtype=torch.int64, device=dev)
        if idx_ids is None:
            idx_ids = torch.empty(max(n_recs, 1), dtype=torch.int64, device=dev)
        t = None
        if table is not None:
            t = C.byref(NxgRecordTable(table.numel(), table.data_ptr() if table.numel() else None))
        o = NxgArchiveIndexes(cap, out_ptr or None, idx_off.data_ptr(), idx_ids.data_ptr(), 0, 0)
        nk = key.numel() if n_keys is None else n_keys
        err = NetidxError()
        try:
            _check(lib().nxg_archive_index_records(self.ctx, key.data_ptr() if nk else None, nk,
                                                   seg_off.data_ptr(), n_recs, t, C.byref(o),
                                                   C.byref(err)), err)
        except CodecError as e:
            e.n_bytes, e.idx_off, e.idx_ids = int(o.n_bytes), idx_off, idx_ids
            raise
        return int(o.n_bytes), idx_off, idx_ids[:n_recs], int(o.n_ids_total)

    def index_records(self, key, seg_off, table=None, out=None):
        """The RecordIndex of every record in one call (add_batch's HashSet loop, writer.rs:
        407-429): record c's index is bytes[idx_off[c]:idx_off[c+1]], its distinct kept Ids in
        order of first occurrence, idx_ids[c] of them. Returns (bytes, idx_off, idx_ids). `out`: a
        uint8 device tensor to write into (all of it is the capacity); without one the call sizes
        first and allocates."""
        import torch
        off = ids = None
        if out is None:
            n, off, ids, _ = self.index_records_into(key, seg_off, table, None, 0)
            out = torch.empty(max(n, 16), dtype=torch.uint8, device=seg_off.device)
            cap = n
        else:
            cap = out.numel()
        n, off, ids, _ = self.index_records_into(key, seg_off, table, out.data_ptr(), cap, off, ids)
        return out[:n], off, ids

    def scan_index(self, dbuf, idx_off, idx_end, keep, buf_len=None):
        """nxg_archive_scan_index (scan_index_at, reader.rs:394-422, for every record of a
        filtered read): dbuf a uint8 device tensor, idx_off / idx_end host sequences (where each
        record's RecordIndex starts and where the record ends), keep a uint8 device tensor indexed
        by archive Id (or None: no Id is kept). Returns (verdict, n_match): a numpy uint8 array of
        INDEX_NONE / INDEX_MATCH / INDEX_ERR_SHORT / INDEX_ERR_FORMAT."""
        off = np.ascontiguousarray(idx_off, dtype=np.uint64)
        end = np.ascontiguousarray(idx_end, dtype=np.uint64)
        n = len(off)
        assert len(end) == n
        verdict = np.zeros(max(n, 1), np.uint8)
        nm, err = C.c_uint64(0), NetidxError()
        n_ids = keep.numel() if keep is not None else 0
        _check(lib().nxg_archive_scan_index(
            self.ctx, dbuf.data_ptr() if hasattr(dbuf, "data_ptr") else dbuf,
            dbuf.numel() if buf_len is None else buf_len, off.ctypes.data, end.ctypes.data, n,
            keep.data_ptr() if n_ids else None, n_ids, verdict.ctypes.data, C.byref(nm),
            C.byref(err)), err)
        return verdict[:n], nm.value

    def oneshot_pack_pathmap_into(self, path_off, path_bytes, keep, out_ptr, cap, sel=None):
        """nxg_oneshot_pack_pathmap into device memory at `out_ptr` (0 / None: size only).
        path_off: int64 device tensor of n_ids + 1 offsets into path_bytes (uint8 device tensor),
        keep: uint8 device tensor of n_ids flags (filter.is_match per Id). Returns (n_bytes, sel,
        n_sel): sel the uint8 device tensor the call wrote, the `keep` of scan_index, the image
        and oneshot_pack_deltas. A CodecError raised here carries n_bytes, n_sel and sel."""
        import torch
        n_ids = max(path_off.numel() - 1, 0)
        if sel is None:
            sel = torch.empty(max(n_ids, 1), dtype=torch.uint8, device=path_off.device)
        p = NxgOneshotPaths(n_ids, path_off.data_ptr() if n_ids else None,
                            path_bytes.data_ptr() if path_bytes is not None and
                            path_bytes.numel() else None)
        o = NxgOneshotPathmap(cap, out_ptr or None, sel.data_ptr(), 0, 0)
        err = NetidxError()
        try:
            _check(lib().nxg_oneshot_pack_pathmap(self.ctx, C.byref(p),
                                                  keep.data_ptr() if n_ids else None,
                                                  C.byref(o), C.byref(err)), err)
        except CodecError as e:
            e.n_bytes, e.n_sel, e.sel = int(o.n_bytes), int(o.n_sel), sel
            raise
        return int(o.n_bytes), sel[:n_ids], int(o.n_sel)

    def oneshot_pack_pathmap(self, path_off, path_bytes, keep, out=None):
        """The filter set and the pathmap section of a oneshot reply shard (oneshot.rs:111-120) in
        one call. Returns (bytes, sel, n_sel): bytes = varint(n_sel) and, per selected Id in
        ascending order, varint(id) varint(len) path (a uint8 tensor on path_off's device). `out`:
        a uint8 device tensor to write into (all of it is the capacity); without one the call
        sizes first and allocates."""
        import torch
        sel = None
        if out is None:
            n, sel, _ = self.oneshot_pack_pathmap_into(path_off, path_bytes, keep, None, 0)
            out = torch.empty(max(n, 16), dtype=torch.uint8, device=path_off.device)
            cap = n
        else:
            cap = out.numel()
        n, sel, n_sel = self.oneshot_pack_pathmap_into(path_off, path_bytes, keep,
                                                       out.data_ptr(), cap, sel)
        return out[:n], sel, n_sel

    def oneshot_pack_deltas_into(self, cols, infos, ts_secs, ts_nanos, sel, heap, out_ptr, cap,
                                 rec_off=None, rec_items=None):
        """nxg_oneshot_pack_deltas into device memory at `out_ptr` (0 / None: size only). cols /
        infos: archive_decode_window's columns and per-record infos (or (row_off, n_rows) pairs);
        ts_secs / ts_nanos: the records' timestamps (host sequences); sel: oneshot_pack_pathmap's
        uint8 device tensor (or None: no Id is kept); heap: the buffer the window was decoded
        from. Returns (n_bytes, rec_off, rec_items, n_items, n_dropped, n_kept_recs); a CodecError
        raised here carries n_bytes, rec_off and rec_items."""
        import torch
        n = len(infos)
        info = (NxgArchiveBatchInfo * max(n, 1))()
        for i, t in enumerate(infos):
            if isinstance(t, NxgArchiveBatchInfo):
                info[i].row_off, info[i].n_rows = t.row_off, t.n_rows
            else:
                info[i].row_off, info[i].n_rows = t[0], t[1]
        secs = np.ascontiguousarray(ts_secs, dtype=np.int64)
        nanos = np.ascontiguousarray(ts_nanos, dtype=np.uint32)
        assert len(secs) == n and len(nanos) == n
        dev = cols.id.device
        if rec_off is None:
            rec_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        if rec_items is None:
            rec_items = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        n_ids = sel.numel() if sel is not None else 0
        o = NxgOneshotDeltas(cap, out_ptr or None, rec_off.data_ptr(), rec_items.data_ptr(),
                             0, 0, 0, 0)
        err = NetidxError()
        try:
            _check(lib().nxg_oneshot_pack_deltas(
                self.ctx, C.byref(cols.s), _heap_ptr(heap), info if n else None, n,
                secs.ctypes.data if n else None, nanos.ctypes.data if n else None,
                sel.data_ptr() if n_ids else None, n_ids, C.byref(o), C.byref(err)), err)
        except CodecError as e:
            e.n_bytes, e.rec_off, e.rec_items = int(o.n_bytes), rec_off, rec_items
            raise
        return (int(o.n_bytes), rec_off, rec_items[:n], int(o.n_items), int(o.n_dropped),
                int(o.n_kept_recs))

    def oneshot_pack_deltas(self, cols, infos, ts_secs, ts_nanos, sel, heap=None, out=None):
        """batch.retain, the empty-record drop and the deltas elements of one window in one call
        (oneshot.rs:146-149). Returns (bytes, rec_off, rec_items, n_dropped, n_kept_recs): record
        i's element  secs nanos varint(items) item...  is bytes[rec_off[i]:rec_off[i+1]] (empty
        when it keeps nothing); the fragments of successive windows concatenate into the deltas
        section behind its count. `out`: a uint8 device tensor to write into (all of it is the
        capacity); without one the call sizes first and allocates."""
        import torch
        off = items = None
        if out is None:
            n, off, items, _, _, _ = self.oneshot_pack_deltas_into(cols, infos, ts_secs, ts_nanos,
                                                                   sel, heap, None, 0)
            out = torch.empty(max(n, 16), dtype=torch.uint8, device=cols.id.device)
            cap = n
        else:
            cap = out.numel()
        n, off, items, _, dropped, kept = self.oneshot_pack_deltas_into(
            cols, infos, ts_secs, ts_nanos, sel, heap, out.data_ptr(), cap, off, items)
        return out[:n], off, items, dropped, kept

    @staticmethod
    def oneshot_shard_layout(pathmap_len, image_len, deltas_len, n_deltas):
        """nxg_oneshot_shard_layout (host arithmetic, no context): the NxgOneshotShardLayout of a
        shard whose sections have these lengths and whose deltas fragments hold n_deltas
        records."""
        lay, err = NxgOneshotShardLayout(), NetidxError()
        _check(lib().nxg_oneshot_shard_layout(pathmap_len, image_len, deltas_len, n_deltas,
                                              C.byref(lay), C.byref(err)), err)
        return lay

    @staticmethod
    def oneshot_reply_head(shard_lens):
        """nxg_oneshot_reply_head (host arithmetic, no context): (head, reply_len), head =
        varint(Lr) varint(n_shards) as bytes; the reply is head + the shards."""
        lens = np.ascontiguousarray(shard_lens, dtype=np.uint64)
        head = (C.c_uint8 * 20)()
        hl, rl, err = C.c_uint32(0), C.c_uint64(0), NetidxError()
        _check(lib().nxg_oneshot_reply_head(lens.ctypes.data if len(lens) else None, len(lens),
                                            head, C.byref(hl), C.byref(rl), C.byref(err)), err)
        return bytes(head[:hl.value]), rl.value

    def oneshot_assemble_shard(self, layout, pathmap, image, frags, out=None):
        """nxg_oneshot_assemble_shard: the shard len_head | pathmap | image | count_head |
        fragments in device memory. pathmap / image / frags: uint8 device tensors (frags a
        sequence, possibly empty). Returns the shard's bytes, a uint8 device tensor (`out`, or a
        new one of layout.shard_len bytes)."""
        import torch
        if out is None:
            out = torch.empty(max(int(layout.shard_len), 16), dtype=torch.uint8,
                              device=pathmap.device)
            cap = int(layout.shard_len)
        else:
            cap = out.numel()
        fr = (NxgOneshotFrag * max(len(frags), 1))()
        for i, f in enumerate(frags):
            fr[i] = NxgOneshotFrag(f.data_ptr() if f.numel() else None, f.numel())
        n, err = C.c_uint64(0), NetidxError()
        _check(lib().nxg_oneshot_assemble_shard(
            self.ctx, C.byref(layout), pathmap.data_ptr() if pathmap.numel() else None,
            image.data_ptr() if image.numel() else None, fr if len(frags) else None, len(frags),
            out.data_ptr(), cap, C.byref(n), C.byref(err)), err)
        return out[:n.value]

    def encoded_len(self, cols, heap=None):
        n, err = C.c_uint64(0), NetidxError()
        _check(lib().nxg_encoded_len(self.ctx, C.byref(cols.s), _heap_ptr(heap), C.byref(n),
                                     C.byref(err)), err)
        return n.value

    def encode_into(self, cols, heap, out_ptr, cap):
        n, err = C.c_uint64(0), NetidxError()
        _check(lib().nxg_encode_updates(self.ctx, C.byref(cols.s), _heap_ptr(heap),
                                        C.c_void_p(out_ptr), cap, C.byref(n), C.byref(err)), err)
        return n.value

    def encode_batch(self, cols, heap=None):
        """Encode columns to one frame payload (torch uint8 tensor on the columns' device)."""
        import torch
        n = self.encoded_len(cols, heap)
        out = torch.empty(max(n, 16), dtype=torch.uint8, device=cols.device)
        m = self.encode_into(cols, heap, out.data_ptr(), n)
        assert m == n
        return out[:n]

    # ---- publisher::To: subscriber write batches ---------------------------------------------
    def decode_writes(self, frame, cols=None, wcols=None, check=True, fast=False):
        """Decode one To frame (Subscribe / Unsubscribe / Write; host bytes or a device tensor):
        returns (Columns, WriteCols). Rows are the Writes, with wcols.wflags / wcols.wid; the
        other messages are control spans. A malformed frame raises PackError(kind, offset) (check);
        last_status() and self.writes_status describe the decode. fast: try the tile-parallel
        fast decoder first (nxg_decode_writes_opts; path PATH_WRITES_FAST when it takes the
        frame, PATH_WRITES after the fallback to the general decoder; the same columns)."""
        n = len(frame) if not hasattr(frame, "numel") else frame.numel()
        if cols is None:
            cols = Columns(n // 5 + 1, n + 1, n // 3 + 1, LAYOUT_MIXED,
                           "cuda" if wcols is None else wcols.device)
        if wcols is None:
            wcols = WriteCols(cols.caps["rows"], cols.device)
        ptr, keep = _frame_ptr(frame)
        st, err = NxgStatus(), NetidxError()
        if fast:
            opts = NxgWriteDecodeOpts(1, 0)
            ok = lib().nxg_decode_writes_opts(self.ctx, C.c_void_p(ptr), n, C.byref(cols.s),
                                              C.byref(wcols.s), C.byref(opts), C.byref(st),
                                              C.byref(err))
        else:
            ok = lib().nxg_decode_writes(self.ctx, C.c_void_p(ptr), n, C.byref(cols.s),
                                         C.byref(wcols.s), C.byref(st), C.byref(err))
        _check(ok, err)
        self.writes_status = st
        if check and st.err_kind:
            raise PackError(st.err_kind, st.err_offset)
        return cols, wcols

    def encoded_writes_len(self, cols, wcols, heap=None):
        n, err = C.c_uint64(0), NetidxError()
        _check(lib().nxg_encoded_writes_len(self.ctx, C.byref(cols.s), C.byref(wcols.s),
                                            _heap_ptr(heap), C.byref(n), C.byref(err)), err)
        return n.value

    def encode_writes_into(self, cols, wcols, heap, out_ptr, cap):
        n, err = C.c_uint64(0), NetidxError()
        _check(lib().nxg_encode_writes(self.ctx, C.byref(cols.s), C.byref(wcols.s),
                                       _heap_ptr(heap), C.c_void_p(out_ptr), cap, C.byref(n),
                                       C.byref(err)), err)
        return n.value

    def encode_writes(self, cols, wcols, heap=None):
        """Encode rows as To::Write messages (control spans: pre-encoded Subscribe / Unsubscribe
        messages in `heap`) to one frame payload, a uint8 tensor on the columns' device."""
        import torch
        n = self.encoded_writes_len(cols, wcols, heap)
        out = torch.empty(max(n, 16), dtype=torch.uint8, device=cols.device)
        if n:
            m = self.encode_writes_into(cols, wcols, heap, out.data_ptr(), n)
            assert m == n
        return out[:n]

    def route_writes(self, table, frame, cols, wcols, row_begin=0, ctl_begin=0, fresh_wid=0,
                     cap_entries=None, cap_wait=None, cap_unsub=None, cap_reply=None):
        """handle_batch_inner's Write and Unsubscribe arms (publisher/server.rs:171-245, 497-576)
        for a decoded To frame: `frame` is the device tensor decode_writes read, `cols` / `wcols`
        what it returned, `table` a WriteTable. Processes rows and control spans from (row_begin,
        ctl_begin) up to the first Subscribe span and returns a WriteRoute (outcome per row,
        per-channel requests, the reply frame, the wait list, the unsubscribed Ids, next_row /
        next_ctl to resume from). Capacities default to the a-priori bounds; one that is exceeded
        raises RouteCapacity carrying the required counts."""
        import torch
        dev = cols.device
        n_rows, n_ctl = int(cols.s.n_rows), int(cols.s.n_ctl)
        rows, spans = max(n_rows - row_begin, 0), max(n_ctl - ctl_begin, 0)
        cap_entries = rows * table.max_fanout if cap_entries is None else cap_entries
        cap_wait = rows if cap_wait is None else cap_wait
        cap_unsub = spans if cap_unsub is None else cap_unsub
        cap_reply = 58 * rows + 12 * spans if cap_reply is None else cap_reply

        def buf(n, dt=torch.int64):
            return torch.empty(max(int(n), 1), dtype=dt, device=dev)

        r = WriteRoute()
        r.outcome = buf(n_rows, torch.uint8)
        r.chan_off = torch.zeros(table.n_chans + 1, dtype=torch.int64, device=dev)
        r.ent_id, r.ent_row = buf(cap_entries), buf(cap_entries)
        r.wait_row, r.wait_id, r.wait_wid = buf(cap_wait), buf(cap_wait), buf(cap_wait)
        r.unsub_id = buf(cap_unsub)
        r.reply = buf(cap_reply, torch.uint8)
        torch.cuda.synchronize(dev)  # (as Columns: the zero fill is done)
        s = r.s
        s.cap_rows, s.outcome = max(n_rows, 1), r.outcome.data_ptr()
        s.disp = NxgDispatch(cap_entries, r.chan_off.data_ptr(), r.ent_id.data_ptr(),
                             r.ent_row.data_ptr(), None, 0, 0)
        s.cap_wait, s.wait_row, s.wait_id, s.wait_wid = (
            cap_wait, r.wait_row.data_ptr(), r.wait_id.data_ptr(), r.wait_wid.data_ptr())
        s.cap_unsub, s.unsub_id = cap_unsub, r.unsub_id.data_ptr()
        s.cap_reply, s.reply = cap_reply, r.reply.data_ptr()
        tb = table.c_struct()
        if not hasattr(frame, "data_ptr") or frame.device.type != "cuda":
            raise CodecError("frame: the device tensor the columns were decoded from")
        ptr = frame.data_ptr()
        err = NetidxError()
        ok = lib().nxg_route_writes(self.ctx, C.byref(tb), C.c_void_p(ptr), C.byref(cols.s),
                                    C.byref(wcols.s), row_begin, ctl_begin, fresh_wid,
                                    C.byref(s), C.byref(err))
        if not ok and err.msg and b"NXG_CAPACITY" in err.msg:
            msg = err.msg.decode()
            lib().nxg_error_free(C.byref(err))
            raise RouteCapacity(msg, r)
        _check(ok, err)
        r.row_begin = row_begin
        return r

    def route_subscribes(self, table, frame, cols, row_begin=0, ctl_begin=0, span_perm=None,
                         cap_sub=None, cap_deferred=None, cap_reply=None):
        """handle_batch_inner's Subscribe arm and subscribe() (publisher/server.rs:60-137, 506-549)
        for one run of consecutive Subscribe spans of a decoded To frame, from span ctl_begin on:
        `frame` is the device tensor decode_writes read, `cols` what it returned, `table` a
        SubscribeTable, `span_perm` None (Anonymous) or a sequence / device tensor of n_ctl
        permission words (SUB_PERM_DENY: Denied). Returns a SubscribeRoute: outcome and Id per
        span, the subscribed (Id, permissions), the deferred spans, the reply frame, next_ctl and
        `stopped` (0 the end, 1 continue with route_writes, 2 a path the host must handle).
        Capacities default to the a-priori bounds; one that is exceeded raises RouteCapacity
        carrying the required counts."""
        import torch
        dev = cols.device
        n_ctl = int(cols.s.n_ctl)
        spans = max(n_ctl - ctl_begin, 0)
        cap_sub = spans if cap_sub is None else cap_sub
        cap_deferred = min(spans, table.deferred_room) if cap_deferred is None else cap_deferred
        if not hasattr(frame, "data_ptr") or frame.device.type != "cuda":
            raise CodecError("frame: the device tensor the columns were decoded from")
        if cap_reply is None:
            cap_reply = frame.numel() + spans * (21 + table.max_value_len)

        def buf(n, dt=torch.int64):
            return torch.empty(max(int(n), 1), dtype=dt, device=dev)

        r = SubscribeRoute()
        r.ctl_begin = ctl_begin
        r.outcome = buf(n_ctl, torch.uint8)
        r.span_id = buf(n_ctl)
        r.sub_id, r.sub_perm = buf(cap_sub), buf(cap_sub, torch.int32)
        r.deferred = buf(cap_deferred)
        r.reply = buf(cap_reply, torch.uint8)
        if span_perm is not None and not hasattr(span_perm, "data_ptr"):
            span_perm = torch.as_tensor(np.array(span_perm, dtype=np.uint32).view(np.int32)).to(dev)
        r.span_perm = span_perm  # (kept alive through the call)
        torch.cuda.synchronize(dev)
        s = r.s
        s.cap_spans, s.outcome, s.span_id = max(n_ctl, 1), r.outcome.data_ptr(), r.span_id.data_ptr()
        s.cap_sub, s.sub_id, s.sub_perm = cap_sub, r.sub_id.data_ptr(), r.sub_perm.data_ptr()
        s.cap_deferred, s.deferred = cap_deferred, r.deferred.data_ptr()
        s.cap_reply, s.reply = cap_reply, r.reply.data_ptr()
        tb = table.c_struct()
        err = NetidxError()
        ok = lib().nxg_route_subscribes(
            self.ctx, C.byref(tb), C.c_void_p(frame.data_ptr()), C.byref(cols.s), row_begin,
            ctl_begin, C.c_void_p(span_perm.data_ptr() if span_perm is not None else 0),
            C.byref(s), C.byref(err))
        if not ok and err.msg and b"NXG_CAPACITY" in err.msg:
            msg = err.msg.decode()
            lib().nxg_error_free(C.byref(err))
            raise RouteCapacity(msg, r)
        _check(ok, err)
        return r

    def route_replies(self, table, frame, cols, row_begin=0, ctl_begin=0, cap_entries=None,
                      cap_sub=None, cap_unsub=None, cap_reply=None):
        """ConnectionCtx::process_batch (subscriber/connection.rs:409-541) for a decoded From frame
        that holds control messages: `frame` is the device tensor decode_into read, `cols` the
        MIXED columns it filled, `table` a ReplyTable. Processes rows and control spans from
        (row_begin, ctl_begin) to the end or to a stop and returns a ReplyRoute (outcome, request
        and Id per span, per-channel entries, last_row, the subscribed and unsubscribed lists, the
        reply frame of To::Unsubscribe messages, next_row / next_ctl / stopped). Capacities default
        to the a-priori bounds; one that is exceeded raises RouteCapacity carrying the required
        counts."""
        import torch
        dev = cols.device
        n_rows, n_ctl = int(cols.s.n_rows), int(cols.s.n_ctl)
        rows, spans = max(n_rows - row_begin, 0), max(n_ctl - ctl_begin, 0)
        cap_entries = (rows + spans) * table.max_fanout if cap_entries is None else cap_entries
        cap_sub = spans if cap_sub is None else cap_sub
        cap_unsub = spans if cap_unsub is None else cap_unsub
        cap_reply = 12 * (rows + spans) if cap_reply is None else cap_reply
        if not hasattr(frame, "data_ptr") or frame.device.type != "cuda":
            raise CodecError("frame: the device tensor the columns were decoded from")

        def buf(n, dt=torch.int64):
            return torch.empty(max(int(n), 1), dtype=dt, device=dev)

        r = ReplyRoute()
        r.row_begin, r.ctl_begin = row_begin, ctl_begin
        r.outcome = buf(n_ctl, torch.uint8)
        r.span_q, r.span_id = buf(n_ctl), buf(n_ctl)
        r.chan_off = torch.zeros(table.subs.n_chans + 1, dtype=torch.int64, device=dev)
        r.ent_sub, r.ent_row = buf(cap_entries), buf(cap_entries)
        r.last_row = buf(table.subs.slot_sub_id.numel())
        r.sub_span, r.sub_q, r.sub_id = buf(cap_sub), buf(cap_sub), buf(cap_sub)
        r.unsub_id, r.unsub_slot = buf(cap_unsub), buf(cap_unsub, torch.int32)
        r.reply = buf(cap_reply, torch.uint8)
        torch.cuda.synchronize(dev)  # (as Columns: the zero fill is done)
        s = r.s
        s.cap_spans = max(n_ctl, 1)
        s.outcome, s.span_q, s.span_id = (r.outcome.data_ptr(), r.span_q.data_ptr(),
                                          r.span_id.data_ptr())
        s.disp = NxgDispatch(cap_entries, r.chan_off.data_ptr(), r.ent_sub.data_ptr(),
                             r.ent_row.data_ptr(), r.last_row.data_ptr(), 0, 0)
        s.cap_sub, s.sub_span, s.sub_q, s.sub_id = (cap_sub, r.sub_span.data_ptr(),
                                                    r.sub_q.data_ptr(), r.sub_id.data_ptr())
        s.cap_unsub, s.unsub_id, s.unsub_slot = (cap_unsub, r.unsub_id.data_ptr(),
                                                 r.unsub_slot.data_ptr())
        s.cap_reply, s.reply = cap_reply, r.reply.data_ptr()
        tb = table.c_struct()
        err = NetidxError()
        ok = lib().nxg_route_replies(self.ctx, C.byref(tb), C.c_void_p(frame.data_ptr()),
                                     C.byref(cols.s), row_begin, ctl_begin, C.byref(s),
                                     C.byref(err))
        if not ok and err.msg and b"NXG_CAPACITY" in err.msg:
            msg = err.msg.decode()
            lib().nxg_error_free(C.byref(err))
            raise RouteCapacity(msg, r)
        _check(ok, err)
        return r

    def decode_range(self, dframe, frame_len, begin, end, cols):
        """Decode the messages that start in [begin, end) of a device frame (rows at cols[0:]);
        returns the NxgRange summary (entry / exit / n_rows / ok)."""
        ptr = dframe.data_ptr() if hasattr(dframe, "data_ptr") else int(dframe)
        rng, err = NxgRange(), NetidxError()
        _check(lib().nxg_decode_range(self.ctx, C.c_void_p(ptr), frame_len, begin, end,
                                      C.byref(cols.s), C.byref(rng), C.byref(err)), err)
        return rng

    def decode_share(self, dframe, frame_len, share, shares, cols):
        """nxg_decode_share: the frame decoded whole, row share `share` of `shares` into cols;
        returns (first row of the share, NxgStatus)."""
        ptr = dframe.data_ptr() if hasattr(dframe, "data_ptr") else int(dframe)
        off, st, err = C.c_uint64(0), NxgStatus(), NetidxError()
        _check(lib().nxg_decode_share(self.ctx, C.c_void_p(ptr), frame_len, share, shares,
                                      C.byref(cols.s), C.byref(off), C.byref(st), C.byref(err)),
               err)
        return off.value, st

    def encode_frames(self, cols, heap, out_ptr, cap, max_frames=16):
        """Encode into out_ptr and return (total length, [frame payload lengths]) as
        WriteChannel::queue_send / try_flush would cut them (MAX_BATCH, channel.rs:177-257)."""
        n, k, err = C.c_uint64(0), C.c_uint64(0), NetidxError()
        chunks = np.zeros(max_frames, np.uint64)
        _check(lib().nxg_encode_frames(self.ctx, C.byref(cols.s), _heap_ptr(heap),
                                       C.c_void_p(out_ptr), cap, C.byref(n),
                                       C.c_void_p(chunks.ctypes.data), max_frames, C.byref(k),
                                       C.byref(err)), err)
        return n.value, [int(x) for x in chunks[: k.value]]

    def encode_async(self, cols, heap, out_ptr, cap):
        """Enqueue an encode; the returned c_uint64 holds the length after sync()."""
        n, err = C.c_uint64(0), NetidxError()
        self.__dict__.setdefault("_pending_len", []).append(n)  # written by the C side at sync
        _check(lib().nxg_encode_updates_async(self.ctx, C.byref(cols.s), _heap_ptr(heap),
                                              C.c_void_p(out_ptr), cap, C.byref(n),
                                              C.byref(err)), err)
        return n


NO_SLOT = 0xFFFFFFFF


class SubTable:
    """Device-resident Id -> subscription table: ConnectionCtx.subscriptions and each Sub's
    sub_id / streams / last (netidx/src/subscriber/connection.rs:54-60), as the CSR arrays of
    include/nxg_codec.h's NxgSubTable. Publisher Ids are dense (netidx-core/src/utils.rs:130-134),
    so the map is a table indexed by Id."""

    def __init__(self, slot_of_id, slot_sub_id, slot_stream_off, stream_chan, slot_has_last,
                 n_chans, device="cuda"):
        import torch

        def t(a, dt):
            return torch.as_tensor(np.array(a, dtype=dt, copy=True)).to(device)

        self.slot_of_id = t(slot_of_id, np.uint32).view(torch.int32)
        self.slot_sub_id = t(slot_sub_id, np.uint64).view(torch.int64)
        self.slot_stream_off = t(slot_stream_off, np.uint32).view(torch.int32)
        self.stream_chan = t(stream_chan, np.uint32).view(torch.int32)
        self.slot_has_last = t(slot_has_last, np.uint8)
        self.n_chans = int(n_chans)
        assert self.slot_stream_off.numel() == self.slot_sub_id.numel() + 1
        assert self.slot_has_last.numel() == self.slot_sub_id.numel()

    @classmethod
    def from_subscriptions(cls, subs, n_chans, n_ids=None, device="cuda"):
        """subs: {id: (sub_id, [chan, ...], keeps_last)} -- one subscription per Id, its streams
        in registration order (handle_connect_stream, connection.rs:320-359)."""
        n_ids = (max(subs) + 1 if subs else 0) if n_ids is None else n_ids
        slot_of_id = np.full(n_ids, NO_SLOT, np.uint32)
        sub_ids, offs, chans, last = [], [0], [], []
        for slot, (i, (sid, streams, keep)) in enumerate(sorted(subs.items())):
            if i < n_ids:
                slot_of_id[i] = slot
            sub_ids.append(sid)
            chans.extend(streams)
            offs.append(len(chans))
            last.append(1 if keep else 0)
        return cls(slot_of_id, np.array(sub_ids, np.uint64), np.array(offs, np.uint32),
                   np.array(chans, np.uint32), np.array(last, np.uint8), n_chans, device)

    def c_struct(self):
        return NxgSubTable(self.slot_of_id.numel(), self.slot_of_id.data_ptr(),
                           self.slot_sub_id.numel(), self.slot_sub_id.data_ptr(),
                           self.slot_stream_off.data_ptr(), self.stream_chan.data_ptr(),
                           self.slot_has_last.data_ptr(), self.n_chans)


class TagView:
    """Device tensors of the type-partitioned view (include/nxg_codec.h NxgTagView): tag t's rows
    are the dense indices [off[t], off[t+1]): row_of (int32 holding u32), fixed (int64), aux
    (int32); rank[i] is row i's index among its tag's rows."""

    def __init__(self, cap, device="cuda"):
        import torch
        self.cap = cap
        self.rank = torch.empty(cap, dtype=torch.int32, device=device)
        self.row_of = torch.empty(cap, dtype=torch.int32, device=device)
        self.fixed = torch.empty(cap, dtype=torch.int64, device=device)
        self.aux = torch.empty(cap, dtype=torch.int32, device=device)
        self.n_rows, self.count, self.off = 0, None, None

    def numpy(self):
        n = self.n_rows
        return {"rank": self.rank[:n].cpu().numpy().view(np.uint32),
                "row_of": self.row_of[:n].cpu().numpy().view(np.uint32),
                "fixed": self.fixed[:n].cpu().numpy().view(np.uint64),
                "aux": self.aux[:n].cpu().numpy().view(np.uint32),
                "count": self.count, "off": self.off}


class Dispatch:
    """Per-channel update batches (by_chan, connection.rs:62-65): channel c's batch is
    (ent_sub, ent_row)[chan_off[c]:chan_off[c+1]], in batch order; last_row[slot] = 1 + the last
    row of the slot's subscription (0: none)."""

    def __init__(self, chan_off, ent_sub, ent_row, last_row, n_entries, n_unmatched):
        self.chan_off, self.ent_sub, self.ent_row, self.last_row = chan_off, ent_sub, ent_row, last_row
        self.n_entries, self.n_unmatched = n_entries, n_unmatched

    def batches(self):
        """{chan: [(sub_id, row), ...]} on the host (non-empty channels only)."""
        off = self.chan_off.cpu().numpy().view(np.uint64)
        sub = self.ent_sub[: self.n_entries].cpu().numpy().view(np.uint64)
        row = self.ent_row[: self.n_entries].cpu().numpy().view(np.uint64)
        return {c: list(zip(sub[off[c]:off[c + 1]].tolist(), row[off[c]:off[c + 1]].tolist()))
                for c in range(len(off) - 1) if off[c + 1] > off[c]}


PUB_UPDATE, PUB_UPDATE_CHANGED, PUB_UPDATE_CLIENT = 0, 1, 2
TAG_UNSUBSCRIBED = 0x40  # archive rows: Event::Unsubscribed


class PubTable:
    """Device-resident publisher state for UpdateBatch::commit (netidx/src/publisher/mod.rs:
    776-845): pb.by_id as a dense slot table (Id -> slot), each slot's subscribed clients (CSR)
    and current value (tag/fixed/aux columns; text, Decimal and Abstract bytes in cur_heap; the
    elements of container values in cur_ctag/cur_cfixed/cur_caux)."""

    def __init__(self, slot_of_id, slot_client_off, client, n_clients, cur_tag, cur_fixed,
                 cur_aux=None, cur_heap=None, device="cuda", cur_ctag=None, cur_cfixed=None,
                 cur_caux=None):
        import torch

        def t(a, dt):
            return torch.as_tensor(np.array(a, dtype=dt, copy=True)).to(device)

        self.slot_of_id = t(slot_of_id, np.uint32).view(torch.int32)
        self.slot_client_off = t(slot_client_off, np.uint32).view(torch.int32)
        self.client = t(client, np.uint32).view(torch.int32)
        self.n_clients = int(n_clients)
        self.cur_tag = None if cur_tag is None else t(cur_tag, np.uint8)
        self.cur_fixed = t(cur_fixed, np.uint64).view(torch.int64)
        self.cur_aux = None if cur_aux is None else t(cur_aux, np.uint32).view(torch.int32)
        self.cur_heap = None if cur_heap is None else t(cur_heap, np.uint8)
        self.cur_ctag = None if cur_ctag is None else t(cur_ctag, np.uint8)
        self.cur_cfixed = None if cur_cfixed is None else t(cur_cfixed, np.uint64).view(torch.int64)
        self.cur_caux = None if cur_caux is None else t(cur_caux, np.uint32).view(torch.int32)

    def c_struct(self):
        def p(x):
            return x.data_ptr() if x is not None and x.numel() else None
        return NxgPubTable(self.slot_of_id.numel(), p(self.slot_of_id),
                           self.slot_client_off.numel() - 1, p(self.slot_client_off),
                           p(self.client), self.n_clients, p(self.cur_tag), p(self.cur_fixed),
                           p(self.cur_aux), p(self.cur_heap), p(self.cur_ctag),
                           p(self.cur_cfixed), p(self.cur_caux))


class ValueCapacity(CodecError):
    """An apply or rebuild whose payload does not fit (NXG_CAPACITY); the table is unchanged.
    `need_bytes` / `need_children`: the new values' payload; `live_bytes` / `live_children`: what
    the table would hold, i.e. what a rebuild into other arrays needs."""

    def __init__(self, msg, res):
        super().__init__(msg)
        self.res = res
        for k, v in res.items():
            setattr(self, k, v)


class ValueTable:
    """A device-resident table of values (NxgValueTable): slot -> value in the columnar form, with
    payload bytes in a heap and container elements in child columns that the table owns (torch
    tensors). `f64`: only `fixed` (NxgPubTable.cur_tag == NULL). `tensors`: caller-made arrays
    (tag, fixed, aux, heap, ctag, cfixed, caux) instead of fresh ones -- they may be longer than
    the stated capacities (the tests' guard bands)."""

    ARRAYS = (("tag", "uint8", "slots"), ("fixed", "int64", "slots"), ("aux", "int32", "slots"),
              ("heap", "uint8", "bytes"), ("ctag", "uint8", "children"),
              ("cfixed", "int64", "children"), ("caux", "int32", "children"))

    def __init__(self, codec, n_slots, cap_bytes=0, cap_children=0, f64=False, device="cuda",
                 tensors=None):
        import torch
        self.codec, self.f64, self.device = codec, bool(f64), torch.device(device)
        self.caps = {"slots": int(n_slots), "bytes": 0 if f64 else int(cap_bytes),
                     "children": 0 if f64 else int(cap_children)}
        self.t = {}
        for name, dt, kind in self.ARRAYS:
            if f64 and name != "fixed":
                self.t[name] = None
            elif tensors is not None:
                self.t[name] = tensors[name]
            else:
                self.t[name] = torch.zeros(max(self.caps[kind], 1), dtype=getattr(torch, dt),
                                           device=self.device)
        self.s = NxgValueTable()
        self.s.n_slots = self.caps["slots"]
        self.s.cap_bytes, self.s.cap_children = self.caps["bytes"], self.caps["children"]
        for name, _, _ in self.ARRAYS:
            setattr(self.s, name, _ptr(self.t[name]).value)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)  # the codec runs on its own stream

    n_slots = property(lambda self: int(self.s.n_slots))
    heap_used = property(lambda self: int(self.s.heap_used))
    heap_live = property(lambda self: int(self.s.heap_live))
    child_used = property(lambda self: int(self.s.child_used))
    child_live = property(lambda self: int(self.s.child_live))

    def counters(self):
        return (self.heap_used, self.heap_live, self.child_used, self.child_live)

    def init(self):
        err = NetidxError()
        _check(lib().nxg_value_table_init(self.codec.ctx, C.byref(self.s), C.byref(err)), err)
        return self

    @staticmethod
    def _finish(ok, err, res):
        if not ok:
            msg = err.msg.decode() if err.msg else "unknown error"
            lib().nxg_error_free(C.byref(err))
            raise (ValueCapacity(msg, res.dict()) if "NXG_CAPACITY" in msg else CodecError(msg))
        return res.dict()

    def apply(self, batch, src_row, heap=None, heap_len=None):
        """Slot s takes the value of batch row src_row[s] - 1 (src_row: n_slots device words,
        Dispatch.last_row as it is). `heap`: the batch's payload bytes (a device tensor; for a
        decoded frame the frame). Returns the NxgValueApply as a dict; ValueCapacity when the
        payload does not fit, CodecError for a refused slot -- the table is unchanged then."""
        if heap_len is None:
            heap_len = 0 if heap is None else heap.numel()
        res, err = NxgValueApply(), NetidxError()
        ok = lib().nxg_value_table_apply(self.codec.ctx, C.byref(self.s), C.byref(batch.s),
                                         _heap_ptr(heap), heap_len, _ptr(src_row),
                                         C.byref(res), C.byref(err))
        return self._finish(ok, err, res)

    def rebuild(self, dst, batch=None, src_row=None, heap=None, heap_len=None):
        """`dst` (another ValueTable, at least as many slots) takes this table's values, the
        selected slots the batch's: compaction, growth, or the apply that did not fit."""
        if heap_len is None:
            heap_len = 0 if heap is None else heap.numel()
        res, err = NxgValueApply(), NetidxError()
        ok = lib().nxg_value_table_rebuild(
            self.codec.ctx, C.byref(self.s), C.byref(batch.s) if batch is not None else None,
            _heap_ptr(heap), heap_len, _ptr(src_row), C.byref(dst.s), C.byref(res),
            C.byref(err))
        return self._finish(ok, err, res)

    def set_unsubscribed(self, slots):
        """The named slots (an int32 device tensor, or a list) become Event::Unsubscribed."""
        import torch
        if not hasattr(slots, "data_ptr"):
            slots = torch.as_tensor(np.array(slots, dtype=np.uint32).view(np.int32)).to(
                self.device)
            torch.cuda.synchronize(self.device)
        err = NetidxError()
        _check(lib().nxg_value_table_set_unsubscribed(self.codec.ctx, C.byref(self.s),
                                                      _ptr(slots) if slots.numel() else None,
                                                      slots.numel(), C.byref(err)), err)

    def as_pub_columns(self):
        """(cur_tag, cur_fixed, cur_aux, cur_heap, cur_ctag, cur_cfixed, cur_caux): the tensors a
        PubTable's current values are (None where the table has none)."""
        n = self.n_slots
        if self.f64:
            return (None, self.t["fixed"][:n], None, None, None, None, None)
        k = self.child_used
        kids = tuple(self.t[x][:k] if k else None for x in ("ctag", "cfixed", "caux"))
        return (self.t["tag"][:n], self.t["fixed"][:n], self.t["aux"][:n],
                self.t["heap"] if self.caps["bytes"] else None) + kids

    def pub_table(self, slot_of_id, slot_client_off, client, n_clients):
        """A PubTable over these arrays (no copy): the commit and the Subscribe replies then read
        what apply wrote."""
        pt = PubTable(slot_of_id, slot_client_off, client, n_clients, None, [0],
                      device=self.device)
        (pt.cur_tag, pt.cur_fixed, pt.cur_aux, pt.cur_heap, pt.cur_ctag, pt.cur_cfixed,
         pt.cur_caux) = self.as_pub_columns()
        return pt

    def as_columns(self, ids):
        """An NxgColumns over the table's rows and children with `ids` (an int64 device tensor of
        n_slots Ids) as the id column: input of nxg_encode_updates, its heap being t["heap"]."""
        v = _ColumnsView()
        v.device = self.device
        v.t = dict(self.t, id=ids)
        v.s = NxgColumns()
        v.s.layout = LAYOUT_F64 if self.f64 else LAYOUT_MIXED
        v.s.mem = MEM_DEVICE
        v.s.cap_rows = v.s.n_rows = self.n_slots
        v.s.cap_children = v.s.n_children = self.child_used
        for name in ("id", "tag", "fixed", "aux", "ctag", "cfixed", "caux"):
            setattr(v.s, name, _ptr(v.t.get(name)).value)
        return v

    def numpy(self):
        """Host copies: the seven arrays (the written part of heap and children) and counters."""
        import torch
        torch.cuda.synchronize(self.device)
        n, hu, ku = self.n_slots, self.heap_used, self.child_used
        cut = {"slots": n, "bytes": hu, "children": ku}
        out = {}
        for name, dt, kind in self.ARRAYS:
            t = self.t[name]
            out[name] = None if t is None else t[:cut[kind]].cpu().numpy().view(
                {"uint8": np.uint8, "int64": np.uint64, "int32": np.uint32}[dt])
        return out


NOT_SUBSCRIBED = 0xFFFFFFFF
PERM_WRITE = 0x04  # Permissions::WRITE (resolver_server/auth.rs:26)
WRITE_ROUTED, WRITE_UNSUBSCRIBED, WRITE_DENIED, WRITE_NOT_ACCEPTED = 0, 1, 2, 3


class WriteTable:
    """Device-resident state of one client for write routing (include/nxg_codec.h NxgWriteTable):
    cl.subscribed as a dense Id -> Permissions table and pb.on_write as Id -> slot plus each slot's
    open channels in list order (CSR), as write() reads them (publisher/server.rs:201-217)."""

    def __init__(self, perm_of_id, slot_of_id, slot_chan_off, chan, n_chans, device="cuda"):
        import torch

        def t(a, dt):
            return torch.as_tensor(np.array(a, dtype=dt, copy=True)).to(device)

        self.perm_of_id = t(perm_of_id, np.uint32).view(torch.int32)
        self.slot_of_id = t(slot_of_id, np.uint32).view(torch.int32)
        offs = np.array(slot_chan_off, dtype=np.uint32)
        self.slot_chan_off = t(offs, np.uint32).view(torch.int32)
        self.chan = t(chan, np.uint32).view(torch.int32)
        self.n_chans = int(n_chans)
        self.n_slots = max(len(offs) - 1, 0)
        self.max_fanout = int((offs[1:].astype(np.int64) - offs[:-1]).max()) if self.n_slots else 0
        assert self.perm_of_id.numel() == self.slot_of_id.numel()

    @classmethod
    def from_state(cls, subscribed, on_write, n_chans, n_ids=None, device="cuda"):
        """subscribed: {id: permission bits} (cl.subscribed); on_write: {id: [open chan, ...]}
        (pb.on_write after the retain of server.rs:207-214). n_ids: the table's extent (default:
        one past the largest Id of either map)."""
        if n_ids is None:
            n_ids = max([-1] + list(subscribed) + list(on_write)) + 1
        perm = np.full(n_ids, NOT_SUBSCRIBED, np.uint32)
        slot_of_id = np.full(n_ids, NO_SLOT, np.uint32)
        for i, p in subscribed.items():
            if i < n_ids:
                perm[i] = p
        offs, chans = [0], []
        for slot, (i, cs) in enumerate(sorted(on_write.items())):
            if i < n_ids:
                slot_of_id[i] = slot
            chans.extend(cs)
            offs.append(len(chans))
        return cls(perm, slot_of_id, offs, chans, n_chans, device)

    def c_struct(self):
        def p(x):
            return x.data_ptr() if x.numel() else None
        return NxgWriteTable(self.perm_of_id.numel(), p(self.perm_of_id), p(self.slot_of_id),
                             self.n_slots, p(self.slot_chan_off), p(self.chan), self.n_chans)


class WriteRoute:
    """What Codec.route_writes returns (include/nxg_codec.h NxgWriteRoute): device tensors
    outcome (per row of the columns), chan_off / ent_id / ent_row (per-channel requests, as
    Dispatch), wait_row / wait_id / wait_wid, unsub_id and reply, with the counts in `s`."""

    def __init__(self):
        self.s = NxgWriteRoute()
        self.row_begin = 0

    def __getattr__(self, k):
        s = self.__dict__.get("s")
        if s is not None and k in ("n_entries", "n_wait", "n_unsub", "n_replies", "reply_len",
                                   "n_fresh", "next_row", "next_ctl"):
            return int(getattr(s, k))
        raise AttributeError(k)

    @property
    def stopped_at_subscribe(self):
        return bool(self.s.stopped_at_subscribe)

    @property
    def n_outcome(self):
        return [int(x) for x in self.s.n_outcome]

    def batches(self):
        """{chan: [(id, row), ...]} on the host (non-empty channels only)."""
        return Dispatch(self.chan_off, self.ent_id, self.ent_row, None, self.n_entries,
                        0).batches()

    def numpy(self):
        """Host copies, trimmed: outcome of the processed rows [row_begin, next_row), the wait
        triples, unsub_id and the reply bytes."""
        u = lambda t, n: t[:n].cpu().numpy().view(np.uint64)
        return {"outcome": self.outcome[self.row_begin:self.next_row].cpu().numpy(),
                "wait": list(zip(u(self.wait_row, self.n_wait).tolist(),
                                 u(self.wait_id, self.n_wait).tolist(),
                                 u(self.wait_wid, self.n_wait).tolist())),
                "unsub_id": u(self.unsub_id, self.n_unsub).tolist(),
                "reply": self.reply[: self.reply_len].cpu().numpy().tobytes()}


class RouteCapacity(CodecError):
    """nxg_route_writes / nxg_route_subscribes: a capacity was exceeded; `route` holds the required
    counts (n_entries, n_wait, n_unsub, reply_len / n_sub, n_deferred, reply_len)."""

    def __init__(self, msg, route):
        super().__init__(msg)
        self.route = route


NO_ID = (1 << 64) - 1
SUB_PERM_DENY = 0xFFFFFFFF
PERM_ALL = 0x3F  # Permissions::all() (resolver_server/auth.rs:24-29)
SUB_SUBSCRIBED, SUB_NO_SUCH_VALUE, SUB_DENIED, SUB_DEFERRED, SUB_IGNORED = 0, 1, 2, 3, 4
MAX_DEFERRED = 1000000  # publisher/server.rs:56


def path_is_plain(path):
    """nxg_path_is_plain: no `\\`, not empty, no `//`, no trailing `/` unless the path is `/`."""
    p = path.encode() if isinstance(path, str) else bytes(path)
    b = (C.c_uint8 * max(len(p), 1)).from_buffer_copy(p + b"\0")
    return bool(lib().nxg_path_is_plain(b, len(p)))


def path_hash(path, offset=0):
    """nxg_path_hash: the word a PathTable stores for the path (never 0 or 1). `offset` places
    the bytes that many bytes into the buffer handed over (the answer does not depend on it)."""
    p = path.encode() if isinstance(path, str) else bytes(path)
    b = (C.c_uint8 * (offset + len(p) + 1)).from_buffer_copy(b"\xa5" * offset + p + b"\xa5")
    return int(lib().nxg_path_hash(C.addressof(b) + offset, len(p)))


def _pack_paths(paths):
    ps = [p.encode() if isinstance(p, str) else bytes(p) for p in paths]
    off = np.zeros(len(ps) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in ps], dtype=np.uint64)
    heap = np.frombuffer(b"".join(ps) or b"\0", np.uint8).copy()
    return ps, heap, off


class PathTable:
    """A device-resident by_path (nxg_path_table_*): path bytes -> publisher::Id, built and queried
    on the GPU. At most cap_paths paths and cap_bytes bytes of paths."""

    def __init__(self, codec, cap_paths, cap_bytes):
        err = NetidxError()
        self.codec = codec
        self.h = lib().nxg_path_table_new(codec.ctx, cap_paths, cap_bytes, C.byref(err))
        if not self.h:
            _check(False, err)

    def close(self):
        if getattr(self, "h", None):
            lib().nxg_path_table_free(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def __len__(self):
        return int(lib().nxg_path_table_len(self.h))

    def insert(self, paths, ids):
        """paths[i] -> ids[i]; returns n_dup (paths already present, or equal to a path earlier
        in the call: the earlier one wins)."""
        ps, heap, off = _pack_paths(paths)
        idv = np.array(ids, dtype=np.uint64)
        assert len(idv) == len(ps)
        dup, err = C.c_uint64(), NetidxError()
        _check(lib().nxg_path_table_insert(self.codec.ctx, self.h, heap.ctypes.data,
                                           off.ctypes.data, idv.ctypes.data, len(ps),
                                           C.byref(dup), C.byref(err)), err)
        return int(dup.value)

    def remove(self, paths):
        """Returns n_missing."""
        ps, heap, off = _pack_paths(paths)
        miss, err = C.c_uint64(), NetidxError()
        _check(lib().nxg_path_table_remove(self.codec.ctx, self.h, heap.ctypes.data,
                                           off.ctypes.data, len(ps), C.byref(miss),
                                           C.byref(err)), err)
        return int(miss.value)

    def lookup_device(self, dheap, doff, dlen, n=None):
        """Device tensors (uint8 bytes, int64 offsets, int32 lengths) -> an int64 device tensor of
        Ids (NO_ID as -1)."""
        import torch
        n = doff.numel() if n is None else n
        out = torch.empty(max(n, 1), dtype=torch.int64, device=doff.device)
        err = NetidxError()
        _check(lib().nxg_path_table_lookup(self.codec.ctx, self.h, _ptr(dheap), _ptr(doff),
                                           _ptr(dlen), n, _ptr(out), C.byref(err)), err)
        return out[:n]

    def lookup(self, paths, device="cuda"):
        """Host paths -> a list of Ids (NO_ID where the table has none)."""
        import torch
        ps, heap, off = _pack_paths(paths)
        if not ps:
            return []
        dheap = torch.from_numpy(heap).to(device)
        doff = torch.from_numpy(off[:-1].view(np.int64).copy()).to(device)
        dlen = torch.from_numpy(np.diff(off).astype(np.uint32).view(np.int32)).to(device)
        out = self.lookup_device(dheap, doff, dlen, len(ps))
        return out.cpu().numpy().view(np.uint64).tolist()


def _value_len(v):
    """|Value::encode| of a (tag, payload) value (the model of tests/golden/make_golden.py)."""
    def vl(x):
        return (((x | 1).bit_length() - 1) * 9 + 73) >> 6
    t, p = v
    if t in (0, 2, 8):
        return 5
    if t in (1, 5):
        return 1 + vl(p)
    if t in (3, 7):
        bits = 32 if t == 3 else 64
        return 1 + vl(((p << 1) ^ (p >> (bits - 1))) & ((1 << bits) - 1))
    if t in (4, 6, 9):
        return 9
    if t in (10, 11):
        return 13
    if t in (12, 13, 18):
        return 1 + vl(len(p)) + len(p)
    if t in (14, 15, 16):
        return 1
    if t == 19:
        return 1 + vl(len(p)) + sum(_value_len(e) for e in p)
    if t == 20:
        return 17
    if t == 21:
        return 1 + vl(len(p)) + sum(_value_len(k) + _value_len(x) for k, x in p)
    if t == 22:
        return 1 + _value_len(p)
    if t in (23, 24):
        return 2
    if t in (25, 26):
        return 3
    if t == 27:
        n = len(p)
        return 1 + n + vl(n + vl(n))
    raise ValueError(t)


def _flatten_value(v, kids, heap):
    """The (tag, fixed, aux) slot of a (tag, payload) value: a container's elements go to `kids`
    in one block, depth-first; text, Decimal and Abstract bytes are appended to `heap`."""
    M = (1 << 64) - 1
    t, p = v
    if t in (2, 3, 6, 7, 24, 26):
        return (t, p & M, 0)
    if t in (0, 1, 4, 5, 8, 9, 23, 25):
        return (t, p, 0)
    if t in (10, 11):
        return (t, p[0] & M, p[1])
    if t in (12, 13, 18, 20, 27):
        off = len(heap)
        heap += p
        return (t, off, len(p))
    if t in (14, 15, 16):
        return (t, 1 if t == 14 else 0, 0)
    if t in (19, 21, 22):
        elems = list(p) if t == 19 else ([x for kv in p for x in kv] if t == 21 else [p])
        base = len(kids)
        kids.extend([None] * len(elems))
        for i, e in enumerate(elems):
            kids[base + i] = _flatten_value(e, kids, heap)
        return (t, base, 1 if t == 22 else len(p))
    raise ValueError(t)


class SubscribeTable:
    """Device-resident publisher state for Subscribe routing (include/nxg_codec.h
    NxgSubscribeTable): by_path (a PathTable), by_id and the current values (a PubTable),
    extended_auth as allow_of_id, the default publishers' bases (sorted) and deferred_room."""

    def __init__(self, paths, pub, allow_of_id=None, defaults=(), deferred_room=MAX_DEFERRED,
                 max_value_len=9, device="cuda"):
        import torch
        self.paths, self.pub = paths, pub
        self.allow_of_id = None if allow_of_id is None else torch.as_tensor(
            np.array(allow_of_id, dtype=np.uint8, copy=True)).to(device)
        bases = sorted(set(b.encode() if isinstance(b, str) else bytes(b) for b in defaults))
        _, heap, off = _pack_paths(bases)
        self.n_defaults = len(bases)
        self.default_heap = torch.from_numpy(heap).to(device)
        self.default_off = torch.from_numpy(off.view(np.int64).copy()).to(device)
        self.deferred_room = int(deferred_room)
        self.max_value_len = int(max_value_len)

    @classmethod
    def from_state(cls, codec, by_path, by_id, n_ids=None, denied_ids=None, defaults=(),
                   deferred_room=MAX_DEFERRED, device="cuda"):
        """by_path: {path bytes: id}; by_id: {id: value}, a value being (tag, payload) as in
        tests/golden/make_golden.py (an Array's payload a list of values, a Map's a list of
        pairs); denied_ids: the Ids extended_auth denies this client (None: no extended_auth);
        defaults: the open default publishers' bases. n_ids: slot_of_id's extent (default: one
        past the largest published Id)."""
        if n_ids is None:
            n_ids = max([-1] + list(by_id)) + 1
        pt = PathTable(codec, max(len(by_path), 1), max(sum(len(p) for p in by_path), 1))
        if by_path:
            items = list(by_path.items())
            pt.insert([p for p, _ in items], [i for _, i in items])
        slot_of_id = np.full(n_ids, NO_SLOT, np.uint32)
        rows, kids, heap = [], [], bytearray()
        for slot, (i, v) in enumerate(sorted(by_id.items())):
            if i < n_ids:
                slot_of_id[i] = slot
            rows.append(_flatten_value(v, kids, heap))
        col = lambda a, k: [x[k] for x in a]
        pub = PubTable(slot_of_id, [0] * (len(rows) + 1), [], 0, col(rows, 0), col(rows, 1),
                       col(rows, 2), np.frombuffer(bytes(heap) or b"\0", np.uint8), device,
                       cur_ctag=col(kids, 0) or [0], cur_cfixed=col(kids, 1) or [0],
                       cur_caux=col(kids, 2) or [0])
        allow = None
        if denied_ids is not None:
            allow = np.ones(n_ids, np.uint8)
            for i in denied_ids:
                if i < n_ids:
                    allow[i] = 0
        mv = max([9] + [_value_len(v) for v in by_id.values()])
        return cls(pt, pub, allow, defaults, deferred_room, mv, device)

    def c_struct(self):
        self._pub = self.pub.c_struct()  # (kept alive: the C struct points at it)
        def p(x):
            return x.data_ptr() if x is not None and x.numel() else None
        return NxgSubscribeTable(self.paths.h, C.addressof(self._pub), p(self.allow_of_id),
                                 self.n_defaults, p(self.default_heap), p(self.default_off),
                                 self.deferred_room)


class SubscribeRoute:
    """What Codec.route_subscribes returns (include/nxg_codec.h NxgSubscribeRoute): device tensors
    outcome / span_id (per span of the columns), sub_id / sub_perm, deferred and reply, with the
    counts in `s`."""

    def __init__(self):
        self.s = NxgSubscribeRoute()
        self.ctl_begin = 0

    def __getattr__(self, k):
        s = self.__dict__.get("s")
        if s is not None and k in ("n_spans", "n_sub", "n_deferred", "n_replies", "reply_len",
                                   "next_ctl", "stopped"):
            return int(getattr(s, k))
        raise AttributeError(k)

    @property
    def n_outcome(self):
        return [int(x) for x in self.s.n_outcome]

    def numpy(self):
        """Host copies, trimmed: outcome and span_id of the run's spans [ctl_begin, next_ctl), the
        subscribed (id, permissions) pairs, the deferred span indices and the reply bytes."""
        u = lambda t, n: t[:n].cpu().numpy().view(np.uint64)
        n_sub = min(self.n_sub, self.sub_id.numel())
        n_def = min(self.n_deferred, self.deferred.numel())
        return {"outcome": self.outcome[self.ctl_begin:self.next_ctl].cpu().numpy().tolist(),
                "span_id": self.span_id[self.ctl_begin:self.next_ctl].cpu().numpy()
                .view(np.uint64).tolist(),
                "sub": list(zip(u(self.sub_id, n_sub).tolist(),
                                self.sub_perm[:n_sub].cpu().numpy().view(np.uint32).tolist())),
                "deferred": u(self.deferred, n_def).tolist(),
                "reply": self.reply[:min(self.reply_len, self.reply.numel())].cpu().numpy()
                .tobytes()}


ENT_SPAN = 1 << 63  # NXG_ENT_SPAN: the entry is Event::Unsubscribed of span ent_row & ~ENT_SPAN
(REPLY_NONE, REPLY_WRITE_RESULT, REPLY_FAILED, REPLY_UNSUBSCRIBED, REPLY_ORPHAN, REPLY_DROPPED,
 REPLY_SUBSCRIBED) = range(7)


class ReplyTable:
    """A connection's state for Codec.route_replies (include/nxg_codec.h NxgReplyTable): `subs` a
    SubTable that also holds one slot per pending request, `pending` a PathTable mapping each
    pending path to its request's index q, pend_slot[q] the request's slot, pend_alive[q] 0 when
    its `finished` receiver is gone (None: all alive)."""

    def __init__(self, subs, pending, pend_slot, pend_alive=None, device="cuda"):
        import torch
        self.subs, self.pending = subs, pending
        self.n_pending = len(pend_slot)
        self.pend_slot = torch.as_tensor(
            np.array(pend_slot, dtype=np.uint32).view(np.int32)).to(device)
        self.pend_alive = None if pend_alive is None else torch.as_tensor(
            np.array(pend_alive, dtype=np.uint8)).to(device)
        off = subs.slot_stream_off.cpu().numpy().view(np.uint32).astype(np.int64)
        self.max_fanout = int(np.diff(off).max()) if len(off) > 1 else 0

    def c_struct(self):
        self._subs = self.subs.c_struct()  # (kept alive through the call)
        return NxgReplyTable(C.addressof(self._subs), self.pending.h, self.n_pending,
                             self.pend_slot.data_ptr() if self.n_pending else None,
                             None if self.pend_alive is None or not self.n_pending
                             else self.pend_alive.data_ptr())


class ReplyRoute:
    """What Codec.route_replies returns (include/nxg_codec.h NxgReplyRoute): device tensors
    outcome / span_q / span_id (per span of the columns), chan_off / ent_sub / ent_row / last_row
    (as Dispatch), sub_span / sub_q / sub_id, unsub_id / unsub_slot and reply, with the counts in
    `s`."""

    def __init__(self):
        self.s = NxgReplyRoute()
        self.row_begin = self.ctl_begin = 0

    def __getattr__(self, k):
        s = self.__dict__.get("s")
        if s is not None and k in ("n_entries", "n_sub", "n_unsub", "n_replies", "reply_len",
                                   "next_row", "next_ctl", "stopped"):
            return int(getattr(s, k))
        raise AttributeError(k)

    @property
    def n_outcome(self):
        return [int(x) for x in self.s.n_outcome]

    @property
    def n_unmatched(self):
        return int(self.s.disp.n_unmatched)

    def batches(self):
        """{chan: [(sub_id, row | ENT_SPAN | span), ...]} on the host (non-empty channels only)."""
        return Dispatch(self.chan_off, self.ent_sub, self.ent_row, self.last_row,
                        min(self.n_entries, self.ent_sub.numel()), self.n_unmatched).batches()

    def numpy(self):
        """Host copies, trimmed to what the call wrote (and to the capacities)."""
        u = lambda t, n: t[:min(n, t.numel())].cpu().numpy().view(np.uint64).tolist()
        k0, k1 = self.ctl_begin, self.next_ctl
        return {"outcome": self.outcome[k0:k1].cpu().numpy().tolist(),
                "span_q": self.span_q[k0:k1].cpu().numpy().view(np.uint64).tolist(),
                "span_id": self.span_id[k0:k1].cpu().numpy().view(np.uint64).tolist(),
                "sub": list(zip(u(self.sub_span, self.n_sub), u(self.sub_q, self.n_sub),
                                u(self.sub_id, self.n_sub))),
                "unsub": list(zip(u(self.unsub_id, self.n_unsub),
                                  self.unsub_slot[:min(self.n_unsub, self.unsub_slot.numel())]
                                  .cpu().numpy().view(np.uint32).tolist())),
                "last_row": self.last_row.cpu().numpy().view(np.uint64).tolist(),
                "reply": self.reply[:min(self.reply_len, self.reply.numel())].cpu().numpy()
                .tobytes()}


def _heap_ptr(heap):
    if heap is None:
        return C.c_void_p(0)
    if hasattr(heap, "data_ptr"):
        return C.c_void_p(heap.data_ptr())
    if isinstance(heap, np.ndarray):
        return C.c_void_p(heap.ctypes.data)
    return C.c_void_p(int(heap))


# ---- host framing (netidx/src/channel.rs) ----------------------------------------------------
class FrameReader:
    """read_task's frame assembly (channel.rs:379-443): feed() the bytes read from a socket in
    any pieces; frames() yields each complete frame payload in order (a copy, as bytes, or
    written into `into`). An encrypted frame raises CodecError("encryption is not supported")."""

    def __init__(self):
        err = NetidxError()
        r = lib().nxg_frame_reader_new(C.byref(err))
        if not r:
            _check(False, err)
        self.r = r

    def close(self):
        if getattr(self, "r", None):
            lib().nxg_frame_reader_free(self.r)
            self.r = None

    def __del__(self):
        self.close()

    def feed(self, data, n=None):
        """Append bytes (bytes, bytearray, memoryview or numpy uint8); `n`: only the first n."""
        if isinstance(data, np.ndarray):
            ptr, size = data.ctypes.data, data.nbytes
        elif isinstance(data, bytes):
            ptr, size = C.cast(C.c_char_p(data), C.c_void_p).value, len(data)
        else:
            mv = memoryview(data).cast("B")
            size = mv.nbytes
            ptr = C.addressof((C.c_uint8 * size).from_buffer(mv)) if size else 0
        size = size if n is None else min(size, int(n))
        err = NetidxError()
        _check(lib().nxg_frame_reader_push(self.r, C.c_void_p(ptr), size, C.byref(err)), err)

    def next_view(self):
        """(address, length) of the next complete payload, valid until the next feed(); None
        if it is not complete yet."""
        p, n, err = C.c_void_p(), C.c_uint64(), NetidxError()
        rc = lib().nxg_frame_reader_next(self.r, C.byref(p), C.byref(n), C.byref(err))
        if rc < 0:
            _check(False, err)
        return (p.value or 0, n.value) if rc == 1 else None

    def frames(self):
        while True:
            v = self.next_view()
            if v is None:
                return
            yield C.string_at(v[0], v[1]) if v[1] else b""

    def buffered(self):
        return lib().nxg_frame_reader_buffered(self.r)


def _msg(fn, *args):
    n = fn(*args, None, 0)
    if n < 0:
        raise CodecError(f"message builder failed ({-n})")
    out = (C.c_uint8 * max(n, 1))()
    m = fn(*args, out, n)
    assert m == n
    return bytes(out[:n])


def msg_subscribe(path, timestamp=0, permissions=0, token=b"", resolver=(0, 0)):
    """To::Subscribe (netproto publisher.rs:57-63) as one len-wrapped message."""
    p = path.encode() if isinstance(path, str) else path
    tok = (C.c_uint8 * max(len(token), 1)).from_buffer_copy(token + b"\0")
    return _msg(lib().nxg_msg_subscribe, p, len(p), resolver[0], resolver[1], timestamp,
                permissions, tok, len(token))


def msg_subscribed(path, id, tag, fixed=0, aux=0, text=b""):
    """From::Subscribed(path, id, scalar value)."""
    p = path.encode() if isinstance(path, str) else path
    t = (C.c_uint8 * max(len(text), 1)).from_buffer_copy(text + b"\0")
    return _msg(lib().nxg_msg_subscribed, p, len(p), id, tag, fixed, aux, t)


def msg_heartbeat():
    return _msg(lib().nxg_msg_heartbeat)


def msg_update(id, tag, fixed=0, aux=0, text=b""):
    """From::Update(id, scalar value) as one len-wrapped message (nxg_msg_update)."""
    t = (C.c_uint8 * max(len(text), 1)).from_buffer_copy(text + b"\0")
    return _msg(lib().nxg_msg_update, id, tag, fixed, aux, t)


def _ip4(ip):
    a = [int(x) for x in ip.split(".")]
    return (a[0] << 24) | (a[1] << 16) | (a[2] << 8) | a[3]


class Resolver:
    """A machine-local anonymous resolver server (nxg_resolver_start): threads in the library."""

    def __init__(self, ip="127.0.0.1", port=0, writer_ttl=120):
        err, bp = NetidxError(), C.c_uint16(0)
        self.h = lib().nxg_resolver_start(ip.encode(), port, C.byref(bp), writer_ttl,
                                          C.byref(err))
        _check(bool(self.h), err)
        self.ip, self.port = ip, bp.value

    def n_published(self):
        return lib().nxg_resolver_n_published(self.h)

    def stop(self):
        if self.h:
            lib().nxg_resolver_stop(self.h)
            self.h = None

    def __del__(self):
        try:
            self.stop()
        except Exception:
            pass


class ResolverClient:
    """A publisher's (write) or subscriber's (read) connection to a resolver."""

    def __init__(self, h, ttl=None):
        self.h, self.ttl = h, ttl

    @classmethod
    def write(cls, ip, port, write_addr):
        err, ttl = NetidxError(), C.c_uint64(0)
        h = lib().nxg_resolver_connect_write(ip.encode(), port, _ip4(write_addr[0]),
                                             write_addr[1], C.byref(ttl), C.byref(err))
        _check(bool(h), err)
        return cls(h, ttl.value)

    @classmethod
    def read(cls, ip, port):
        err = NetidxError()
        h = lib().nxg_resolver_connect_read(ip.encode(), port, C.byref(err))
        _check(bool(h), err)
        return cls(h)

    def publish(self, path):
        p = path.encode() if isinstance(path, str) else path
        err = NetidxError()
        _check(lib().nxg_resolver_publish(self.h, p, len(p), C.byref(err)), err)

    def resolve(self, path):
        """NxgResolved; publisher address as ("a.b.c.d", port) in .addr"""
        p = path.encode() if isinstance(path, str) else path
        r, err = NxgResolved(), NetidxError()
        _check(lib().nxg_resolver_resolve(self.h, p, len(p), C.byref(r), C.byref(err)), err)
        ip = r.publisher_ipv4
        r.addr = (f"{ip >> 24}.{(ip >> 16) & 255}.{(ip >> 8) & 255}.{ip & 255}", r.publisher_port)
        return r

    def close(self):
        if self.h:
            lib().nxg_resolver_client_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def msg_parse(buf, to=False):
    """Parse one control message (publisher::From, or To with to=True); returns NxgCtlMsg."""
    b = bytes(buf)
    a = (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b + b"\0")
    m, err = NxgCtlMsg(), NetidxError()
    _check(lib().nxg_msg_parse(a, len(b), 1 if to else 0, C.byref(m), C.byref(err)), err)
    return m


class Session:
    """One publisher<->subscriber connection (nxg_session_*, include/nxg_codec.h): the handshake,
    frames, the device data path. Blocking; use one thread per session."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def connect(cls, ip, port):
        err = NetidxError()
        h = lib().nxg_session_connect(ip.encode(), port, C.byref(err))
        _check(bool(h), err)
        return cls(h)

    @classmethod
    def listen(cls, ip="127.0.0.1", port=0):
        err, bp = NetidxError(), C.c_uint16(0)
        h = lib().nxg_session_listen(ip.encode(), port, C.byref(bp), C.byref(err))
        _check(bool(h), err)
        s = cls(h)
        s.port = bp.value
        return s

    def accept(self):
        err = NetidxError()
        h = lib().nxg_session_accept(self.h, C.byref(err))
        _check(bool(h), err)
        return Session(h)

    def close(self):
        if self.h:
            lib().nxg_session_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self):
        a = (C.c_uint64 * 4)()
        lib().nxg_session_stats(self.h, a)
        return dict(zip(("frames_in", "bytes_in", "frames_out", "bytes_out"), list(a)))

    def send(self, payload):
        b = bytes(payload)
        a = (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b + b"\0")
        err = NetidxError()
        _check(lib().nxg_session_send(self.h, a, len(b), C.byref(err)), err)

    def recv_frame(self):
        """The next frame's payload (a copy)."""
        p, n, err = C.c_void_p(), C.c_uint64(), NetidxError()
        _check(lib().nxg_session_recv_frame(self.h, C.byref(p), C.byref(n), C.byref(err)), err)
        return C.string_at(p.value, n.value) if n.value else b""

    def recv_decode(self, codec, cols, flags=0):
        """The next frame decoded on the device; returns (NxgStatus, frame length)."""
        st, n, err = NxgStatus(), C.c_uint64(), NetidxError()
        _check(lib().nxg_session_recv_decode(self.h, codec.ctx, C.byref(cols.s), flags,
                                             C.byref(st), C.byref(n), C.byref(err)), err)
        return st, n.value

    def publish(self, codec, cols, heap=None):
        """Device columns encoded on the GPU and written as frames; returns the bytes sent."""
        n, err = C.c_uint64(), NetidxError()
        _check(lib().nxg_session_publish(self.h, codec.ctx, C.byref(cols.s), _heap_ptr(heap),
                                         C.byref(n), C.byref(err)), err)
        return n.value


def range_link(ranges, frame_len):
    """nxg_range_link: row offsets of consecutive byte-range summaries, or (None, bad_index)
    when range `bad_index` does not enter the chain where its predecessor leaves it."""
    n = len(ranges)
    arr = (NxgRange * max(n, 1))(*[r if isinstance(r, NxgRange) else NxgRange.of(r)
                                   for r in ranges])
    offs = np.zeros(max(n, 1), np.uint64)
    bad, err = C.c_uint32(0), NetidxError()
    ok = lib().nxg_range_link(arr, n, frame_len, C.c_void_p(offs.ctypes.data), C.byref(bad),
                              C.byref(err))
    if err.msg:
        lib().nxg_error_free(C.byref(err))
    return (offs[:n], None) if ok else (None, int(bad.value))


_AG = C.CFUNCTYPE(C.c_bool, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
_AGV = C.CFUNCTYPE(C.c_bool, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32,
                   C.c_uint32)
_ELEN = C.CFUNCTYPE(C.c_bool, C.c_void_p, C.POINTER(NxgColumns), C.c_void_p,
                    C.POINTER(C.c_uint64))
_ENC = C.CFUNCTYPE(C.c_bool, C.c_void_p, C.POINTER(NxgColumns), C.c_void_p, C.c_void_p,
                   C.c_uint64, C.POINTER(C.c_uint64))
_DRNG = C.CFUNCTYPE(C.c_bool, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                    C.POINTER(NxgColumns), C.POINTER(NxgRange))
_DSHR = C.CFUNCTYPE(C.c_bool, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                    C.POINTER(NxgColumns), C.POINTER(C.c_uint64), C.POINTER(NxgStatus))


class NxgCommOps(C.Structure):
    _fields_ = [("user", C.c_void_p), ("allgather", _AG), ("allgatherv", _AGV),
                ("encoded_len", _ELEN), ("encode", _ENC), ("decode_range", _DRNG),
                ("decode_share", _DSHR)]


def _guard(fn):
    """A Python callback behind a C function pointer: an exception becomes `false` (the library
    then agrees the failure with the other ranks) after it is printed."""
    def call(*a):
        try:
            r = fn(*a)
            return True if r is None else bool(r)
        except Exception:  # noqa: BLE001 -- reported, then turned into the C failure code
            import traceback
            traceback.print_exc()
            return False
    return call


class Comm:
    """Communicator of the sharded calls (one process per GPU): RCCL (nxg_comm_init), or a
    caller-provided transport and optional local codec (nxg_comm_init_ops, Comm.with_ops)."""

    @staticmethod
    def unique_id():
        buf, err = (C.c_uint8 * 128)(), NetidxError()
        _check(lib().nxg_comm_unique_id(C.byref(buf), C.byref(err)), err)
        return bytes(buf)

    def __init__(self, codec, nranks, rank, uid):
        err = NetidxError()
        b = (C.c_uint8 * 128).from_buffer_copy(uid)
        self.h = lib().nxg_comm_init(codec.ctx, nranks, rank, C.byref(b), C.byref(err))
        _check(self.h is not None, err)
        self.codec, self.nranks, self.rank = codec, nranks, rank

    @classmethod
    def with_ops(cls, codec, nranks, rank, allgather, allgatherv, encoded_len=None, encode=None,
                 decode_range=None, decode_share=None):
        """nxg_comm_init_ops. allgather(mine: bytes) -> bytes of every rank's, in rank order;
        allgatherv(buf_ptr, offsets, nranks, rank) fills every shard of the buffer at its
        offset. The optional local codec: encoded_len(NxgColumns) -> int; encode(NxgColumns,
        out_ptr, cap) -> int; decode_range(frame_ptr, frame_len, begin, end, NxgColumns) ->
        (begin, end, entry, exit, n_rows, ok, err_kind); and, optionally with it,
        decode_share(frame_ptr, frame_len, share, shares, NxgColumns) -> (row_off, n_rows,
        err_kind, err_offset). codec may be None with the codec."""
        self = cls.__new__(cls)

        def ag(user, mine, all_, nbytes):
            got = allgather(C.string_at(mine, nbytes))
            assert len(got) == nbytes * nranks
            C.memmove(all_, got, len(got))

        def agv(user, buf, off, n, r):
            allgatherv(int(buf or 0), [int(off[i]) for i in range(n + 1)], int(n), int(r))

        fns = [_AG(_guard(ag)), _AGV(_guard(agv))]
        if decode_range is not None:
            def elen(user, cols, heap, out):
                out[0] = int(encoded_len(cols.contents))

            def enc(user, cols, heap, out, cap, n):
                n[0] = int(encode(cols.contents, int(out or 0), int(cap)))

            def drng(user, frame, flen, b, e, cols, rng):
                t = decode_range(int(frame or 0), int(flen), int(b), int(e), cols.contents)
                rng[0] = t if isinstance(t, NxgRange) else NxgRange.of(t)

            fns += [_ELEN(_guard(elen)), _ENC(_guard(enc)), _DRNG(_guard(drng))]
        else:
            fns += [_ELEN(), _ENC(), _DRNG()]
        if decode_share is not None:
            def dshr(user, frame, flen, share, shares, cols, off, st):
                o, nr, ek, eo = decode_share(int(frame or 0), int(flen), int(share), int(shares),
                                             cols.contents)
                off[0] = int(o)
                st[0] = NxgStatus(n_rows=int(nr), err_kind=int(ek), err_offset=int(eo))

            fns.append(_DSHR(_guard(dshr)))
        else:
            fns.append(_DSHR())
        self._fns = fns  # the C function pointers live as long as the communicator
        self.ops = NxgCommOps(None, *fns)
        err = NetidxError()
        self.h = lib().nxg_comm_init_ops(codec.ctx if codec else None, nranks, rank,
                                         C.byref(self.ops), C.byref(err))
        _check(self.h is not None, err)
        self.codec, self.nranks, self.rank = codec, nranks, rank
        return self

    def _ctx(self):
        return self.codec.ctx if self.codec else None

    def close(self):
        if getattr(self, "h", None):
            lib().nxg_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode_allgather(self, cols, heap, out_ptr, cap):
        """Every rank's shard into one frame on every rank; returns (length, shard offsets)."""
        n, err = C.c_uint64(0), NetidxError()
        offs = np.zeros(self.nranks, np.uint64)
        cs = cols.s if hasattr(cols, "s") else cols
        _check(lib().nxg_encode_allgather(self._ctx(), self.h, C.byref(cs),
                                          _heap_ptr(heap), C.c_void_p(out_ptr), cap, C.byref(n),
                                          C.c_void_p(offs.ctypes.data), C.byref(err)), err)
        return n.value, [int(x) for x in offs]

    def decode_sharded(self, dframe, frame_len, cols):
        """This rank's byte range of one frame (or, for a frame the byte-range decoders decline,
        its row share: rng.ok == 2); returns (first global row, NxgRange)."""
        ptr = dframe.data_ptr() if hasattr(dframe, "data_ptr") else int(dframe)
        off, rng, err = C.c_uint64(0), NxgRange(), NetidxError()
        cs = cols.s if hasattr(cols, "s") else cols
        _check(lib().nxg_decode_sharded(self._ctx(), self.h, C.c_void_p(ptr), frame_len,
                                        C.byref(cs), C.byref(off), C.byref(rng),
                                        C.byref(err)), err)
        return off.value, rng


def frame_split(msg_lens):
    """Frame payload lengths for a queue of encoded messages (WriteChannel::queue_send)."""
    a = np.ascontiguousarray(msg_lens, np.uint64)
    out = np.zeros(len(a) + 1, np.uint64)
    n = lib().nxg_frame_split(a.ctypes.data, len(a), out.ctypes.data, len(out))
    if n < 0:
        raise CodecError("message exceeds MAX_BATCH")
    return out[:n]


def frame_header(payload_len, encrypted=False):
    b = (C.c_uint8 * 4)()
    lib().nxg_frame_header(payload_len, encrypted, b)
    return bytes(b)


def frame_parse_header(buf):
    ln, enc = C.c_uint32(0), C.c_bool(False)
    a = np.frombuffer(bytes(buf), np.uint8)
    n = lib().nxg_frame_parse_header(a.ctypes.data, len(a), C.byref(ln), C.byref(enc))
    return (None if n == 0 else (ln.value, bool(enc.value)))


def columns_from_arrays(id, fixed, tag=None, aux=None, ctag=None, cfixed=None, caux=None,
                        ctl_row=None, ctl_off=None, ctl_len=None, ctl_variant=None,
                        device="cuda"):
    """Build encode-input Columns from host numpy arrays (uploaded to `device`)."""
    import torch
    n = len(id)
    nc = 0 if ctag is None else len(ctag)
    nk = 0 if ctl_row is None else len(ctl_row)
    layout = LAYOUT_F64 if tag is None else LAYOUT_MIXED
    cols = Columns(n, nc, nk, layout, device)

    def put(name, arr, dt):
        if arr is None or len(arr) == 0:
            return
        src = torch.from_numpy(np.ascontiguousarray(arr).view(dt))
        cols.t[name][: len(arr)].copy_(src)

    put("id", id, np.int64)
    put("fixed", fixed, np.int64)
    put("tag", tag, np.uint8)
    put("aux", aux, np.int32)
    put("ctag", ctag, np.uint8)
    put("cfixed", cfixed, np.int64)
    put("caux", caux, np.int32)
    put("ctl_row", ctl_row, np.int64)
    put("ctl_off", ctl_off, np.int64)
    put("ctl_len", ctl_len, np.int32)
    put("ctl_variant", ctl_variant, np.uint8)
    cols.s.n_rows, cols.s.n_children, cols.s.n_ctl = n, nc, nk
    return cols
