// nxg_decode_f64_seq_backlog.hip -- the backlog kernel of nxg_decode_f64_seq.hip as an object of
// its own: the same source, built with the flags the Makefile gives this file (the reason stands
// there, next to NXG_F64S_BACKLOG_TU).
#define NXG_F64S_BACKLOG_TU 1
#include "nxg_decode_f64_seq.hip"
