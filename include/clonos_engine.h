/*
 * clonos_engine.h -- C-ABI of the MI355X causal-log engine (libclonos_engine.so).
 *
 * This is the drop-in boundary a JNI layer binds.  Plain
 * pointers and sizes only; no exceptions cross it; every entry point returns an
 * int status (CLG_OK == 0).  clg_last_error() gives a thread-local message.
 *
 * Reference interfaces replaced (R/ = /root/reference/flink-runtime/src/main/java/
 * org/apache/flink/runtime/causal/):
 *   ThreadCausalLog      R/log/thread/ThreadCausalLog.java:33-96  (impl :51-527)
 *   JobCausalLog         R/log/job/JobCausalLog.java:50-78        (impl JobCausalLogImpl.java:71-300)
 *   DeterminantEncoder   R/determinant/DeterminantEncoder.java:28-65 (decode side; impl
 *                        SimpleDeterminantEncoder.java:78-342)
 *   DeterminantResponseEvent.merge  R/DeterminantResponseEvent.java:128-148
 *
 * Memory model: log bytes live in HBM in fixed-size segments (= Netty components of
 * determinantBufferSize bytes, NettyConfig.java:86-89); log metadata (epoch start
 * offsets, consumer offsets, visible writer index) lives in the host engine and is
 * updated with exactly the reference's semantics.  Outputs go to caller-allocated
 * buffers, either host (CLG_MEM_HOST) or device (CLG_MEM_DEVICE, a hipMalloc'd pointer
 * on the engine's device).  Entry points are safe to call from any thread.  Per-log calls
 * (append, hasDelta, offset, a slice served from the host tail, logLength, a host-input
 * upstream delta) take only their log's lock stripe; GPU and multi-log calls take the
 * engine lock and every stripe.  GPU work runs on the engine stream, apart from device
 * slices with CLG_F_ASYNC_SLICE, which run on a second (gather) stream.
 */
#ifndef CLONOS_ENGINE_H
#define CLONOS_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLG_ABI_VERSION 6

/* ---- status codes ---------------------------------------------------------- */
enum {
  CLG_OK = 0,
  CLG_E_INVALID_ARG = -1,
  CLG_E_CORRUPT_TAG = -2,        /* CorruptDeterminantArrayException(tag)  SimpleDeterminantEncoder.java:92 */
  CLG_E_TRUNCATED = -3,          /* record runs past the span (ByteBuf IndexOutOfBounds) */
  CLG_E_BAD_ENUM = -4,           /* Type.values()[ord] / CheckpointType.values()[ord] out of range (:231, :285) */
  CLG_E_NEG_LEN = -5,            /* negative name / reference length (NegativeArraySizeException, :235, :282) */
  CLG_E_BAD_SERIAL = -6,         /* malformed Java serialization stream (type 3, :333-341) */
  CLG_E_CONSUMER_BACKWARDS = -7, /* "Consumer went backwards"  ThreadCausalLogImpl.java:215-218 */
  CLG_E_NO_CONSUMER = -8,        /* getOffset/getDelta before hasDelta (NPE at :245 / :256) */
  CLG_E_GAP = -9,                /* upstream delta leaves a gap (delta.readerIndex(<0) at :143) */
  CLG_E_NOSPACE = -10,           /* segment pool exhausted (Java side blocks: requestBufferBlocking :444) */
  CLG_E_CAPACITY = -11,          /* caller output buffer too small; required size reported */
  CLG_E_STATE = -12,             /* inconsistent log state (index out of bounds) */
  CLG_E_DEVICE = -13,            /* HIP runtime error */
  CLG_E_NO_LOG = -14,            /* unknown / closed log handle */
  CLG_E_NOT_BUFFER_BUILT = -15,  /* subpartition recovery buffer holds another determinant
                                    (RuntimeException, ReplayingState.java:172-177) */
  CLG_E_EPOCH_GAP = -16          /* in-flight replay reaches an epoch with no buffers (the reference's
                                    ReplayIterator NPEs at logToReplay.get(++currentKey), :133) */
};

/* CLG_MEM_MAPPED: host memory registered with clg_host_register.  For decode outputs
 * (clg_decoded.out_kind) the single-launch small decode writes it straight from the GPU (no
 * staging copy), and so do the column kernels for clg_columns.out_kind; clg_columnize also reads
 * a decoded batch from it (clg_decoded.out_kind of its input), and the pack kernels read columns
 * from it and write clg_packed's arrays to it.  Every other path treats it as CLG_MEM_HOST. */
enum { CLG_MEM_HOST = 0, CLG_MEM_DEVICE = 1, CLG_MEM_MAPPED = 2 };

/* Pin and map [p, p + bytes) of host memory for the device (hipHostRegister, mapped); a
 * caller that keeps its output buffers across decodes registers them once.  Unregister
 * before the memory is freed. */
int clg_host_register(void* p, uint64_t bytes);
int clg_host_unregister(void* p);

/* Determinant tags (Determinant.java:23-34). */
enum {
  CLG_TAG_ORDER = 0, CLG_TAG_TIMESTAMP = 1, CLG_TAG_RNG = 2, CLG_TAG_SERIALIZABLE = 3,
  CLG_TAG_TIMER_TRIGGER = 4, CLG_TAG_SOURCE_CHECKPOINT = 5, CLG_TAG_IGNORE_CHECKPOINT = 6,
  CLG_TAG_BUFFER_BUILT = 7
};

#define CLG_FULL_SHARING (-1) /* ExecutionConfig.determinantSharingDepth default */

/* ---- identities ---------------------------------------------------------------- */
/* InputChannelID (an AbstractID: lower/upper longs). */
typedef struct clg_channel_id { uint64_t lo, hi; } clg_channel_id;

/* CausalLogID (CausalLogID.java:38-198): main-thread log of a vertex, or a
 * subpartition log {vertex, intermediate result partition (lower, upper), index}. */
typedef struct clg_causal_log_id {
  int16_t vertex_id;
  uint8_t is_main;
  int8_t subpartition;
  uint32_t reserved;
  int64_t irp_lower;
  int64_t irp_upper;
} clg_causal_log_id;

typedef struct clg_config {
  uint32_t segment_bytes;  /* determinantBufferSize (NettyConfig.java:86-89); 16384 by default */
  uint32_t pool_segments;  /* segments preallocated in HBM (pool = segment_bytes * pool_segments);
                              beside it, for segments up to 64 KiB, the Serializable records' positions
                              per segment (segment_bytes / 16 + 8 bytes each, ~6 %; none if HBM is short) */
  int32_t device;          /* HIP device ordinal */
  int32_t sharing_depth;   /* determinantSharingDepth (-1 = full sharing, 0 = logging off) */
  uint32_t flags;          /* CLG_F_* */
  uint32_t host_tail_bytes; /* flushed bytes of each log's tail also kept in host memory (16384 by
                               default): host-output slices / getDeterminants inside the tail are
                               served by memcpy, without a GPU round trip; 0: every slice gathers */
  /* The in-flight (data) log's own HBM pool (InMemorySubpartitionInFlightLogger keeps the
   * network buffers it was given; here their bytes are copied into this pool, apart from
   * the determinant segments so that data volume never starves appendDeterminant).  0:
   * defaults (32 KiB segments = Flink's memory segment size, 4096 of them). */
  uint32_t ifl_segment_bytes;
  uint32_t ifl_pool_segments;
} clg_config;

#define CLG_F_TIMING 1u        /* record per-kernel HIP event timings (clg_kernel_stats) */
#define CLG_F_ROBUST_DECODE 2u /* skip the fast three-pass decode; always use the robust
                                  multi-pass pipeline (the fallback the fused kernel aborts to) */
#define CLG_F_NO_SMALL_DECODE 8u /* batches up to 1 MiB also take the three-pass decode, not the
                                   single-launch small-batch one (tests of the three-pass path) */
#define CLG_F_ASYNC_SLICE 4u   /* slices into device memory (clg_slice_batch, CLG_MEM_DEVICE)
                                  return once queued on the engine's gather stream and overlap
                                  later decodes; the output is ready after clg_sync or once
                                  clg_gather_stream's work completes.  Default: synchronous */

typedef struct clg_engine clg_engine;

/* ---- engine ---------------------------------------------------------------------- */
void clg_config_default(clg_config* cfg);
int clg_engine_create(const clg_config* cfg, clg_engine** out);
void clg_engine_destroy(clg_engine* e);
const char* clg_last_error(void);
int clg_abi_version(void);
/* The HIP stream (hipStream_t) all engine work is issued on. */
void* clg_engine_stream(clg_engine* e);
/* The stream CLG_F_ASYNC_SLICE gathers run on (hipStream_t). */
void* clg_gather_stream(clg_engine* e);
/* Flush staged appends to HBM and wait for all queued GPU work. */
int clg_sync(clg_engine* e);
/* Segments in use / free in the HBM pool. */
int clg_pool_stats(clg_engine* e, uint32_t* used, uint32_t* free_segments);
/* Segments in use / free in the in-flight log's pool. */
int clg_ifl_pool_stats(clg_engine* e, uint32_t* used, uint32_t* free_segments);

/* ---- JobCausalLog scope ------------------------------------------------------------
 * One JobCausalLogImpl per job per TaskManager (JobCausalLogFactory.java:56-67,
 * JobCausalLogImpl.java:71-122): a job owns its thread logs, its sharing depth
 * (ExecutionConfig.determinantSharingDepth) and its latestCompletedCheckpoint.  Job 0 is
 * the engine's default job (sharing depth from clg_config); clg_job_open adds others, so
 * that several jobs on one TaskManager share an engine without sharing log identities or
 * checkpoint CAS state.  Log handles are global to the engine. */
int clg_job_open(clg_engine* e, uint64_t job_lo, uint64_t job_hi, int32_t sharing_depth, uint32_t* job);
/* Closes every log of the job (JobCausalLogImpl.close :277-283); job 0 stays open. */
int clg_job_close(clg_engine* e, uint32_t job);

/* ---- ThreadCausalLog --------------------------------------------------------------- */
/* Opens a log of `job` (ThreadCausalLogImpl ctor :94-112): one empty component is allocated. */
int clg_log_open(clg_engine* e, uint32_t job, const clg_causal_log_id* id, uint32_t* handle);
/* close() :317-328 (the engine does not wait for consumers; caller guarantees drain). */
int clg_log_close(clg_engine* e, uint32_t log);
int clg_log_find(clg_engine* e, uint32_t job, const clg_causal_log_id* id, uint32_t* handle);
/* The CausalLogID and job of an open log (e.g. one clg_process_delta opened). */
int clg_log_get_id(clg_engine* e, uint32_t log, clg_causal_log_id* id, uint32_t* job);
/* appendDeterminant :158-177.  `rec` holds ONE encoded determinant (encodeTo bytes;
 * n == getEncodedSizeInBytes).  Staged on the host, flushed to HBM in batches.  When the
 * append crosses the log's staging bound it also flushes; CLG_E_DEVICE from that flush
 * means the record WAS logged (staged) and only the write-behind failed. */
int clg_append(clg_engine* e, uint32_t log, int64_t epoch, const uint8_t* rec, uint32_t n);
/* Many appends at once: rec i = bytes[off[i], off[i]+len[i]) for log[i] in epoch[i]. */
int clg_append_batch(clg_engine* e, const uint32_t* log, const int64_t* epoch, const uint64_t* off,
                     const uint32_t* len, uint32_t n, const uint8_t* bytes);
/* processUpstreamDelta :117-154 (dedup by offsetFromEpoch, append the new suffix). */
int clg_upstream_delta(clg_engine* e, uint32_t log, int64_t epoch, int32_t offset_from_epoch,
                       const uint8_t* delta, uint32_t n);
/* Batched processUpstreamDelta over one buffer (host or device memory): delta i is
 * bytes[src_off, src_off + len) for log `log`; per-request status.  Device input (an
 * RCCL receive buffer) is scattered into the log segments without a host round trip. */
typedef struct clg_delta_req {
  uint32_t log;
  int32_t offset_from_epoch;
  int64_t epoch;
  uint64_t src_off;
  uint32_t len;
  int32_t status; /* out */
} clg_delta_req;
int clg_upstream_delta_batch(clg_engine* e, clg_delta_req* reqs, uint32_t n, const uint8_t* bytes,
                             uint32_t in_kind);
int clg_log_length(clg_engine* e, uint32_t log, int32_t* out);                                /* :180-192 */
/* logLength of n logs at once (out[i] for log[i]); *total = their sum (either may be NULL). */
int clg_log_length_batch(clg_engine* e, const uint32_t* log, uint32_t n, int32_t* out, uint64_t* total);
int clg_has_delta(clg_engine* e, uint32_t log, clg_channel_id c, int64_t epoch, int32_t* out); /* :196-240 */
int clg_offset_from_epoch(clg_engine* e, uint32_t log, clg_channel_id c, int32_t* out);       /* :243-246 */
/* getDeltaForConsumer :249-277: bytes copied into `out` (host or device).  With
 * CLG_E_CAPACITY, *n is the required size and the consumer has not advanced. */
int clg_get_delta(clg_engine* e, uint32_t log, clg_channel_id c, int64_t epoch, void* out,
                  uint32_t cap, uint32_t out_kind, uint32_t* n);
/* getDeterminants(startEpoch) :285-313 (CLG_E_CAPACITY: *n = required size). */
int clg_get_determinants(clg_engine* e, uint32_t log, int64_t start_epoch, void* out, uint32_t cap,
                         uint32_t out_kind, uint32_t* n);
int clg_notify_checkpoint_complete(clg_engine* e, uint32_t log, int64_t checkpoint_id); /* :398-435 */
int clg_unregister_consumer(clg_engine* e, uint32_t log, clg_channel_id c);              /* :331-336 */

/* State introspection (for parity tests and the JNI safety assertions). */
typedef struct clg_log_state {
  int32_t writer;        /* visibleWriterIndex */
  int32_t capacity;      /* composite capacity = components * segment_bytes */
  int32_t n_components;
  int32_t n_epochs;
} clg_log_state;
int clg_log_get_state(clg_engine* e, uint32_t log, clg_log_state* st, int64_t* epoch_ids,
                      int32_t* epoch_offsets, int32_t cap_epochs);
int clg_consumer_state(clg_engine* e, uint32_t log, clg_channel_id c, int32_t* exists,
                       int64_t* epoch, int32_t* offset);
/* Raw physical bytes of the log's composite (reads HBM). */
int clg_log_read_phys(clg_engine* e, uint32_t log, int32_t phys, uint32_t n, uint8_t* host_out);

/* ---- batched delta slicing (serializeThreadDelta loop, Flat/Grouping serde) ------------
 * For each request, in order: hasDeltaForConsumer; if true, getOffsetFromEpochForConsumer
 * then getDeltaForConsumer.  All deltas are gathered by ONE kernel into `out`
 * (packed in request order).  res[i].status != 0 reports a per-request error
 * (e.g. CLG_E_CONSUMER_BACKWARDS) without aborting the batch. */
typedef struct clg_slice_req {
  uint32_t log;
  uint32_t reserved;
  clg_channel_id consumer;
  int64_t epoch;
} clg_slice_req;
typedef struct clg_slice_res {
  int32_t status;
  int32_t has_delta;
  int32_t offset_from_epoch;
  int32_t len;
  uint64_t out_off;
} clg_slice_res;
int clg_slice_batch(clg_engine* e, const clg_slice_req* reqs, uint32_t n, clg_slice_res* res,
                    void* out, uint64_t cap, uint32_t out_kind, uint64_t* total);
/* Consumer offsets set directly (used to position consumers mid-epoch in benchmarks and
 * when a standby takes over a channel); epoch must exist. */
int clg_consumer_seek(clg_engine* e, uint32_t log, clg_channel_id c, int64_t epoch, int32_t offset);
/* Batched form: consumer reqs[i] of log reqs[i].log positioned at offsets[i] of epoch
 * reqs[i].epoch (stops at the first failing entry). */
int clg_consumer_seek_batch(clg_engine* e, const clg_slice_req* reqs, const int32_t* offsets, uint32_t n);

/* ---- checkpoint completion fan-out (JobCausalLogImpl.notifyCheckpointComplete :230-246) --
 * CAS on the job's latestCompletedCheckpoint; if newer, truncates every open log of that
 * job (other jobs' logs are untouched).  Queued asynchronous decodes (clg_decode_logs_async)
 * whose start epochs are all >= checkpoint_id stay queued: the truncation drops only bytes
 * below the checkpoint, and the segments it frees return to the pool once those decodes are
 * waited for.  A queued decode from an earlier epoch (or appends not yet flushed) is
 * completed first, as by any other call that needs the engine exclusively. */
int clg_truncate_all(clg_engine* e, uint32_t job, int64_t checkpoint_id, int32_t* applied);

/* ---- batched decode (SimpleDeterminantEncoder.decodeNext over whole spans) -------------
 * Output is a dense SoA over all spans (span order, record order):
 *   off[i]  byte offset of record i inside its span;  tag[i];  v0[i] =
 *   ORDER channel (sign-extended byte) | TIMESTAMP ts | RNG number | BUFFER_BUILT bytes |
 *   TIMER_TRIGGER timestamp | SOURCE_CHECKPOINT checkpointID | IGNORE_CHECKPOINT
 *   checkpointID | SERIALIZABLE java-stream length.
 * Wide records (tags 3,4,5,6) also get a side-table row:
 *   w_idx (global record index), w_rc (recordCount), w_v1 (SourceCheckpoint timestamp),
 *   w_var_off/w_var_len (name, storage reference or java stream, span-relative),
 *   w_sub (TimerTrigger type ordinal; SourceCheckpoint type | hasRef<<7). */
typedef struct clg_decoded {
  uint32_t* off;
  uint8_t* tag;
  int64_t* v0;
  uint32_t* w_idx;
  int32_t* w_rc;
  int64_t* w_v1;
  uint32_t* w_var_off;
  uint32_t* w_var_len;
  uint8_t* w_sub;
  uint64_t cap;       /* capacity of the record arrays */
  uint64_t wcap;      /* capacity of the side-table arrays */
  uint32_t out_kind;  /* CLG_MEM_HOST / CLG_MEM_DEVICE */
  uint32_t reserved;
  /* results */
  uint64_t n_rec;
  uint64_t n_wide;
  int32_t err_status; /* first decode error (lowest span), CLG_OK if none */
  uint32_t err_span;
  int64_t err_off;    /* span-relative offset of the failing record */
  int32_t err_tag;
  uint32_t reserved2;
} clg_decoded;

/* Decode spans of host memory: span i = bytes[span_off[i], span_off[i]+span_len[i]).
 * span_rec_base (optional, n+1 entries) receives each span's first record index. */
int clg_decode_host(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off,
                    const uint64_t* span_len, uint32_t n, clg_decoded* out, uint64_t* span_rec_base);
/* Decode logs resident in HBM: span i = getDeterminants(start_epoch[i]) of log[i]
 * (no copy: kernels read the segments in place). */
int clg_decode_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                    clg_decoded* out, uint64_t* span_rec_base);
/* Asynchronous clg_decode_logs: returns once the decode is queued on the engine stream, so
 * the caller can plan and queue other work (e.g. the slices of the same step, or the next
 * batch's decode) while it runs.  `out`, its arrays and span_rec_base must stay valid, and
 * are not to be read, until the clg_decode_wait that pairs with this call returns, which
 * completes the decode (fallback paths included) and returns its status.  Every other call
 * that needs the engine exclusively completes the pending decodes first (their statuses are
 * kept for clg_decode_wait); clg_slice_batch into device memory with CLG_F_ASYNC_SLICE, the
 * consumer seeks, and clg_truncate_all at or below every start epoch leave them pending.
 * Up to CLG_DECODE_MAX_INFLIGHT decodes may be queued before the first is waited for, so the
 * GPU runs decode i+1 while the host completes decode i; give each its own output arrays.
 * One more is CLG_E_STATE (no decode's status is ever dropped). */
#define CLG_DECODE_MAX_INFLIGHT 2
int clg_decode_logs_async(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                          clg_decoded* out, uint64_t* span_rec_base);
/* Completes the OLDEST decode clg_decode_logs_async queued and not yet waited for, and
 * returns ITS status (FIFO: one wait per queued decode, in queue order).  A later decode
 * still running on the GPU is not waited for.  With nothing queued: CLG_OK. */
int clg_decode_wait(clg_engine* e);

/* ---- typed replay columns -----------------------------------------------------------------
 * The stable partition of a decoded batch by determinant class: what LogReplayerImpl
 * (LogReplayerImpl.java:61-119) consumes one typed value at a time -- replayNextChannel a byte,
 * replayRandomInt an int, replayNextTimestamp a long -- and SubpartitionRecoveryThread as int
 * sizes, without the 13-byte rows around them.
 *   class 0 ORDER (tag 0)         order        i8[n_class[0]]
 *   class 1 TIMESTAMP (tag 1)     timestamp    i64[n_class[1]]
 *   class 2 RNG (tag 2)           rng          i32[n_class[2]]
 *   class 3 BUFFER_BUILT (tag 7)  buffer_built i32[n_class[3]]
 *   class 4 WIDE (tags 3,4,5,6)   clg_decoded's side rows (w_idx the global record index), and
 *                                 w_v0[k] = v0[w_idx[k]]
 * Each column holds v0 of its class's records in record order, narrowed to the field's own
 * width (lossless: the decode sign-extends those fields into v0).  tag[n_rec] is the decode's,
 * in record order: it is the interleaving.  span_base[(n_spans + 1) * 5], always host memory
 * (may be NULL): span_base[s * 5 + c] = class-c records before span s, so span s's channels are
 * order[span_base[s*5] .. span_base[(s+1)*5]); an empty span has equal rows; the last row holds
 * the totals.  `off` is not part of the columns: a caller that needs offsets keeps using the
 * decode.  Nothing else is lost: walking tag and popping each class's next value gives back
 * tag, v0 and the side table. */
#define CLG_COL_CLASSES 5
enum { CLG_COL_ORDER = 0, CLG_COL_TIMESTAMP = 1, CLG_COL_RNG = 2, CLG_COL_BUFFER_BUILT = 3, CLG_COL_WIDE = 4 };
typedef struct clg_columns {
  uint8_t* tag;
  int8_t* order;
  int64_t* timestamp;
  int32_t* rng;
  int32_t* buffer_built;
  uint32_t* w_idx;
  int32_t* w_rc;
  int64_t* w_v1;
  uint32_t* w_var_off;
  uint32_t* w_var_len;
  uint8_t* w_sub;
  int64_t* w_v0;
  uint64_t* span_base;        /* host memory, (n_spans + 1) * 5 entries, or NULL */
  uint64_t cap_tag;           /* capacities in elements; a NULL column holds nothing */
  uint64_t cap_order;
  uint64_t cap_timestamp;
  uint64_t cap_rng;
  uint64_t cap_buffer_built;
  uint64_t cap_wide;          /* of each w_* array */
  uint32_t out_kind;          /* CLG_MEM_HOST / CLG_MEM_DEVICE / CLG_MEM_MAPPED (all columns) */
  uint32_t reserved;
  /* results */
  uint64_t n_rec;
  uint64_t n_class[CLG_COL_CLASSES]; /* the class totals */
  int32_t err_status;         /* as clg_decoded: the decode's first error, CLG_OK if none */
  uint32_t err_span;
  int64_t err_off;
  int32_t err_tag;
  uint32_t reserved2;
} clg_columns;

/* Columns of a decoded batch: in->tag, v0, w_* (n_rec records, n_wide side rows; in->off is
 * not read) are device memory, or registered host memory with in->out_kind CLG_MEM_MAPPED;
 * span_rec_base (host, n_spans + 1 entries, not decreasing, the last at most n_rec) is the
 * decode's.  Every column pointer NULL: sizes only (the totals and span_base are filled, no
 * column is written).  A column whose capacity is below its total: CLG_E_CAPACITY with the
 * totals and span_base filled and no column written.  A tag above 7: CLG_E_INVALID_ARG with the
 * lowest such record index in err_off (err_tag the tag, err_span its span), nothing written.
 * Side rows that do not match the wide tags (n_wide): CLG_E_INVALID_ARG.  CLG_MEM_DEVICE and
 * CLG_MEM_MAPPED columns are written by the kernels; CLG_MEM_HOST ones through engine staging
 * and a copy.  Synchronous. */
int clg_columnize(clg_engine* e, const clg_decoded* in, const uint64_t* span_rec_base, uint32_t n_spans,
                  clg_columns* out);
/* clg_decode_logs / clg_decode_host into engine-owned device scratch (kept between calls; grown
 * and decoded again on the decode's own CLG_E_CAPACITY), then clg_columnize.  Ranges, flush rules
 * and decode errors are the decodes': with a decode error each span's records up to its first
 * error are columnized, the error fields are passed through and the decode's status is
 * returned.  Synchronous; pending asynchronous decodes are completed first. */
int clg_decode_logs_columns(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                            clg_columns* out);
int clg_decode_host_columns(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len,
                            uint32_t n, clg_columns* out);
/* The same columns on the CPU (no engine, no GPU): every array of `in` and `out` is host memory;
 * results and error rules are clg_columnize's. */
int clg_columnize_host(const clg_decoded* in, const uint64_t* span_rec_base, uint32_t n_spans, clg_columns* out);

/* ---- the payload column ---------------------------------------------------
 * The columns carry a wide record's payload (a TimerTrigger's name, a SourceCheckpoint's storage
 * reference, a Serializable record's stream) as w_var_off / w_var_len, offsets into its span's
 * bytes.  The payload column carries the bytes: wide rows 0 .. n_rows, row k of span s when
 * row_base[s] <= k < row_base[s + 1] (row_base: host memory, n_spans + 1 entries from 0, not
 * decreasing, the last n_rows; for columns span_base[s * 5 + 4]), give
 *   pos u64[n_rows + 1]  the exclusive prefix sum of w_var_len, pos[n_rows] = n_var
 *   var u8[n_var]        var[pos[k] : pos[k + 1]] = span_s[w_var_off[k] : w_var_off[k] + w_var_len[k]]
 * the shape of clg_encode_in's `var` (w_var_off = pos).  A row of length 0 occupies nothing.  A
 * row whose range passes its span's end: CLG_E_INVALID_ARG, the lowest such row in bad_row,
 * nothing written (no byte of such a row is loaded).  var and pos both NULL: sizes only (n_rows
 * and n_var filled).  cap_var < n_var or cap_pos < n_rows + 1: CLG_E_CAPACITY, the results
 * filled, nothing written. */
typedef struct clg_payloads {
  uint8_t* var;
  uint64_t* pos;
  uint64_t cap_var;           /* bytes */
  uint64_t cap_pos;           /* entries */
  uint32_t out_kind;          /* CLG_MEM_HOST / CLG_MEM_DEVICE / CLG_MEM_MAPPED (both arrays) */
  uint32_t reserved;
  /* results */
  uint64_t n_rows;
  uint64_t n_var;
  uint64_t bad_row;           /* ~0 when none */
} clg_payloads;

/* Payloads of spans bytes[span_off[s], span_off[s] + span_len[s]) of one buffer.  in_kind
 * (CLG_MEM_HOST / CLG_MEM_DEVICE) holds for bytes, w_var_off and w_var_len alike; host input is
 * staged.  span_off, span_len and row_base are host memory.  Synchronous. */
int clg_gather_payloads(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len,
                        uint32_t n_spans, const uint32_t* w_var_off, const uint32_t* w_var_len,
                        const uint64_t* row_base, uint32_t in_kind, clg_payloads* out);
/* Span i is getDeterminants(start_epoch[i]) of log[i], read in place from the segment pool;
 * ranges and flush rules are clg_decode_logs'.  in_kind holds for w_var_off and w_var_len. */
int clg_gather_payloads_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                             const uint32_t* w_var_off, const uint32_t* w_var_len, const uint64_t* row_base,
                             uint32_t in_kind, clg_payloads* out);
/* clg_decode_logs_columns / clg_decode_host_columns, then the payloads of the wide rows they
 * produced, under one engine guard: the columns and the payloads describe the same bytes.  The
 * columns' results, errors and statuses are the existing calls'; that status is returned when it
 * is not CLG_OK, else the payloads'.  With a decode error the payloads are those of the rows
 * kept (each span up to its first error).  When the columns report CLG_E_CAPACITY the payloads'
 * n_rows and n_var are still filled (nothing is written), so one failed call sizes both. */
int clg_decode_logs_columns_var(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                                clg_columns* out, clg_payloads* var);
int clg_decode_host_columns_var(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off,
                                const uint64_t* span_len, uint32_t n, clg_columns* out, clg_payloads* var);
/* The same payloads on the CPU (no engine, no GPU): every array is host memory. */
int clg_gather_payloads_host(const uint8_t* bytes, const uint64_t* span_off, const uint64_t* span_len,
                             uint32_t n_spans, const uint32_t* w_var_off, const uint32_t* w_var_len,
                             const uint64_t* row_base, clg_payloads* out);

/* ---- packed typed columns --------------------------------------------------
 * The five narrow columns bit-packed on the device, so that what crosses the link is the bits the
 * values hold: block-wise frame of reference, 1024 values a block (clonos_amd/csrc/pack.h is the
 * format's one definition).  Five streams, each the clg_columns array of the same name:
 *   CLG_PACK_TAG          tag          u8   FOR
 *   CLG_PACK_ORDER        order        i8   FOR
 *   CLG_PACK_TIMESTAMP    timestamp    i64  DELTA
 *   CLG_PACK_RNG          rng          i32  FOR
 *   CLG_PACK_BUFFER_BUILT buffer_built i32  FOR
 * A stream of n values is ceil(n / 1024) independent blocks, each of 1024 values but the last.
 * All arithmetic is on values sign-extended to 64 bits (tags zero-extended), modulo 2^64.  For a
 * block x_0 .. x_{m-1}:
 *   FOR    residuals r_i = x_i, k = m, first = 0
 *   DELTA  first = x_0, residuals r_i = x_i - x_{i-1} for i = 1 .. m-1, k = m - 1
 *   ref    the minimum residual compared as int64 (0 when k = 0)
 *   range  the maximum residual minus ref, in uint64; width = 0 if range == 0, else 64 - clz(range)
 *   p_i    (uint64)r_i - (uint64)ref, below 2^width
 * The block's payload is the k * width bit little-endian bit string with p_i in bits
 * [i * width, (i + 1) * width) -- bit j is bit j % 64 of the little-endian u64 word j / 64 --
 * zero-padded to 16 * ceil(k * width / 128) bytes: the packed bytes are a pure function of the
 * columns.  desc holds one clg_pack_block per block, stream c's at desc[blk_base[c] ..
 * blk_base[c + 1]); bits holds all payloads back to back in stream order, then block order, so
 * every pos is a multiple of 16.  The wide rows, span_base and the payload column are not
 * packed.  LogReplayerImpl pops one typed value at a time (LogReplayerImpl.java:61-119): a cursor
 * over the blocks serves it without unpacking whole arrays. */
#define CLG_PACK_STREAMS 5
#define CLG_PACK_BLOCK 1024
enum { CLG_PACK_TAG = 0, CLG_PACK_ORDER = 1, CLG_PACK_TIMESTAMP = 2, CLG_PACK_RNG = 3, CLG_PACK_BUFFER_BUILT = 4 };
typedef struct clg_pack_block {
  int64_t ref;
  int64_t first;
  uint64_t pos;    /* byte offset of the block's payload in bits */
  uint32_t width;  /* 0 .. 64 */
  uint32_t count;  /* the block's values, 1 .. 1024 */
} clg_pack_block;
typedef struct clg_packed {
  clg_pack_block* desc;
  uint8_t* bits;
  uint64_t cap_desc;      /* blocks */
  uint64_t cap_bits;      /* bytes */
  uint32_t out_kind;      /* CLG_MEM_HOST / CLG_MEM_DEVICE / CLG_MEM_MAPPED (both arrays) */
  uint32_t reserved;
  /* results */
  uint64_t n_val[CLG_PACK_STREAMS];
  uint64_t blk_base[CLG_PACK_STREAMS + 1];
  uint64_t n_bits;        /* bytes used of bits */
} clg_packed;

/* Pack in->tag (n_rec values), order, timestamp, rng and buffer_built (n_class[0 .. 3] values);
 * nothing else of `in` is read.  in->out_kind says where the five arrays live: device memory and
 * registered host memory (CLG_MEM_MAPPED) are read in place, host memory is staged.  desc and bits
 * both NULL: sizes only (the results are filled, nothing is written).  cap_desc or cap_bits too
 * small: CLG_E_CAPACITY with the results filled and nothing written to the caller (the totals are
 * read from pinned memory and checked before the write pass, as clg_columnize does).
 * CLG_MEM_DEVICE and CLG_MEM_MAPPED outputs (16-byte aligned) are written by the kernels;
 * CLG_MEM_HOST ones through engine staging and one copy each.  Synchronous; the kernels' time is
 * the stat "pack_columns". */
int clg_pack_columns(clg_engine* e, const clg_columns* in, clg_packed* out);
/* clg_decode_logs_columns_var / clg_decode_host_columns_var with the five narrow columns delivered
 * packed: decode and columnize run into engine-owned device scratch (kept between calls), then the
 * pack.  In `wide` the five narrow column pointers must be NULL (CLG_E_INVALID_ARG otherwise); its
 * w_* arrays (all NULL: the wide rows are sized, not delivered), span_base, the totals and the
 * error fields are filled exactly as clg_decode_logs_columns_var fills them.  var may be NULL;
 * otherwise it is the payload column of the same rows.  Ranges, flush rules, decode errors and
 * statuses are the existing calls': each span's records up to its first error are packed and the
 * decode's status is returned.  A capacity failure of any of the three outputs fills every size
 * and writes nothing.  One engine guard covers the whole call. */
int clg_decode_logs_columns_packed(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                                   clg_columns* wide, clg_payloads* var, clg_packed* out);
int clg_decode_host_columns_packed(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off,
                                   const uint64_t* span_len, uint32_t n, clg_columns* wide, clg_payloads* var,
                                   clg_packed* out);
/* The same bytes on the CPU (no engine, no GPU; a measure pass, then the write once the sizes are
 * known to fit): every array is host memory. */
int clg_pack_columns_host(const clg_columns* in, clg_packed* out);
/* `count` values of `stream` from value index `first` into out, in the stream's own element type
 * (u8, i8, i64, i32, i32); only the blocks that range covers are touched.  What is read is
 * validated, for the bytes may come from another process: width <= 64, count in 1 .. 1024 and
 * 1024 for every block but the stream's last, pos + size <= n_bits, blk_base consistent with
 * n_val, and every value inside the stream's type: CLG_E_INVALID_ARG otherwise. */
int clg_unpack_columns_host(const clg_packed* in, uint32_t stream, uint64_t first, uint64_t count, void* out);

/* ---- packed typed columns as input -----------------------------------------
 * A clg_packed read as input: desc, bits, n_val, blk_base and n_bits as a pack filled them, with
 * cap_desc >= blk_base[5] and cap_bits >= n_bits; out_kind names where desc and bits live.  The
 * bytes may come from another process, so nothing is trusted (clonos_amd/csrc/pack.h holds the
 * rules once, for the CPU version and the kernels).  What is wrong is reported in clg_unpack_bad:
 * when several kinds are present the first in the enum's order is reported, with the lowest
 * (stream, block) of that kind; block counts within its stream.
 *   LAYOUT  blk_base[0] != 0, blk_base decreases, blk_base[c + 1] - blk_base[c] is not
 *           ceil(n_val[c] / 1024) (stream: the lowest such c), a capacity below its total or a
 *           null array that would be read (stream 0); block is 0
 *   BLOCK   width > 64, count not 1024 (the stream's last block: what is left), pos + size >
 *           n_bits, or pos not a multiple of 16 (clg_unpack_columns_host does not test that last
 *           rule and is unchanged).  Blocks may lie in any payload order and may share payload bytes
 *   VALUE   an unpacked value outside its stream's type (timestamps always pass)
 * With what == NONE, stream is 0 and block ~0. */
enum { CLG_UNPACK_BAD_NONE = 0, CLG_UNPACK_BAD_LAYOUT = 1, CLG_UNPACK_BAD_BLOCK = 2, CLG_UNPACK_BAD_VALUE = 3,
       CLG_UNPACK_BAD_TOTAL = 4 /* the packed payload column's totals (4.11) */ };
typedef struct clg_unpack_bad { uint32_t what; uint32_t stream; uint64_t block; } clg_unpack_bad;  /* 16 bytes */

/* The whole unpack on the device: out->tag / order / timestamp / rng / buffer_built are written
 * under their cap_* and out->out_kind, n_rec and n_class[0 .. 3] are filled from n_val; w_*,
 * span_base, n_class[4] and the err_* fields are left alone.  The order of the checks: the layout
 * (CLG_E_INVALID_ARG), then the sizes are filled; all five pointers NULL: sizes only (CLG_OK, no
 * descriptor is read); a capacity below its total (a NULL column holds nothing): CLG_E_CAPACITY
 * with the sizes filled and nothing written; then every block and value: CLG_E_INVALID_ARG with
 * `bad` (may be NULL) filled and NOTHING written to the caller's arrays, whatever their kind.
 * Input: CLG_MEM_DEVICE and CLG_MEM_MAPPED are read in place (bits 16-byte aligned, desc 8-byte
 * aligned, else CLG_E_INVALID_ARG); CLG_MEM_HOST is staged with one copy each.  Output: device
 * and registered arrays, aligned to their element (else CLG_E_INVALID_ARG), are written by the
 * kernel; host arrays through engine scratch and one copy each.  No byte outside [0, n_val[c]) of
 * a column is written.  Synchronous; takes the engine guard; the kernels' time is the stat
 * "unpack_columns". */
int clg_unpack_columns(clg_engine* e, const clg_packed* in, clg_columns* out, clg_unpack_bad* bad);
/* The same call on the CPU (no engine, no GPU): every array is host memory and the kinds are not
 * read.  Results, statuses and `bad` are clg_unpack_columns'. */
int clg_unpack_columns_all_host(const clg_packed* in, clg_columns* out, clg_unpack_bad* bad);

/* ---- packed wide rows -------------------------------------------------------
 * The seven w_* arrays packed after a stable partition of the rows by record kind, so that one
 * stream holds one kind of number (clonos_amd/csrc/pack_wide.h is the format's one definition).
 * A row's kind is tag[w_idx[k]] - 3: 0 SERIALIZABLE, 1 TIMER_TRIGGER, 2 SOURCE_CHECKPOINT,
 * 3 IGNORE_CHECKPOINT.  26 streams, each cut into blocks of CLG_PACK_BLOCK values that are packed
 * exactly as a clg_packed block is (ref / first / width, little-endian bit string, 16-byte
 * padding, payloads in stream order and then block order):
 *   0                KIND     the kind of every row       u8   FOR
 *   1                IDX      w_idx of every row          u32  DELTA
 *   2 + 6 * kind + 0 RC       w_rc of that kind's rows    i32  FOR
 *   2 + 6 * kind + 1 V1       w_v1                        i64  DELTA
 *   2 + 6 * kind + 2 VAR_OFF  w_var_off                   u32  DELTA
 *   2 + 6 * kind + 3 VAR_LEN  w_var_len                   u32  FOR
 *   2 + 6 * kind + 4 SUB      w_sub                       u8   FOR
 *   2 + 6 * kind + 5 V0       w_v0                        i64  FOR for kind 0, DELTA for kinds 1-3
 * u8 and u32 elements are zero-extended to 64 bits, i32 sign-extended.  Rank r of kind t is the
 * r-th row of that kind; every field of every kind is packed, so any w_* content round-trips. */
#define CLG_WPACK_KINDS 4
#define CLG_WPACK_FIELDS 6
#define CLG_WPACK_STREAMS 26
enum { CLG_WPACK_KIND = 0, CLG_WPACK_IDX = 1 };
enum { CLG_WPACK_RC = 0, CLG_WPACK_V1 = 1, CLG_WPACK_VAR_OFF = 2, CLG_WPACK_VAR_LEN = 3, CLG_WPACK_SUB = 4, CLG_WPACK_V0 = 5 };
typedef struct clg_packed_wide {
  clg_pack_block* desc;
  uint8_t* bits;
  uint64_t cap_desc;      /* blocks */
  uint64_t cap_bits;      /* bytes */
  uint32_t out_kind;      /* CLG_MEM_HOST / CLG_MEM_DEVICE / CLG_MEM_MAPPED (both arrays) */
  uint32_t reserved;
  /* results */
  uint64_t n_val[CLG_WPACK_STREAMS];
  uint64_t blk_base[CLG_WPACK_STREAMS + 1];
  uint64_t n_bits;        /* bytes used of bits */
  uint64_t bad_row;       /* the lowest row with w_idx >= n_rec or a tag outside 3 .. 6; ~0: none */
} clg_packed_wide;

/* Pack the wide rows of `in`: in->tag (n_rec values) and the seven w_* arrays (n_class[4] rows)
 * are read under in->out_kind; nothing else of `in` is.  The rules are clg_pack_columns': desc and
 * bits both NULL is the sizes-only call; a capacity below its total is CLG_E_CAPACITY with the
 * results filled and nothing written; device and registered memory are read and written in place,
 * host memory goes through engine staging; a misaligned array is CLG_E_INVALID_ARG.  A row whose
 * w_idx is at or past n_rec, or whose tag is outside 3 .. 6: CLG_E_INVALID_ARG with the lowest such
 * row in bad_row and nothing written.  Synchronous; takes the engine guard; the kernels' time is
 * the stat "pack_wide". */
int clg_pack_wide(clg_engine* e, const clg_columns* in, clg_packed_wide* out);
/* The same bytes and rules on the CPU (no engine, no GPU): every array is host memory. */
int clg_pack_wide_host(const clg_columns* in, clg_packed_wide* out);
/* The way back on the CPU: the seven w_* arrays of `out` are written under cap_wide and n_class[4]
 * is filled; nothing else of `out` is touched.  All seven pointers NULL: sizes only.  The input is
 * not trusted; the checks run in clg_unpack_columns_all_host's order and invalid input writes
 * nothing.  LAYOUT, beyond that call's rules: n_val[KIND] != n_val[IDX] (stream 1), the six streams
 * of one kind with different n_val (the lowest stream that differs from its kind's RC), the four
 * kinds' n_val not summing to n_val[KIND] (stream 0).  VALUE, beyond the type bounds (u32: 0 ..
 * 2^32 - 1): a KIND value above 3, and a histogram of KIND that differs from the kinds' n_val
 * (reported with stream 0, block 0). */
int clg_unpack_wide_host(const clg_packed_wide* in, clg_columns* out, clg_unpack_bad* bad);
/* clg_decode_logs_columns_packed / clg_decode_host_columns_packed with the wide rows delivered
 * packed as well: no plain wide row is copied to the caller.  All twelve column pointers of `sizes`
 * must be NULL (CLG_E_INVALID_ARG otherwise); its span_base, the totals and the error fields are
 * filled as clg_decode_logs_columns_packed fills them.  var may be NULL.  When it is given,
 * var->var non-NULL with var->pos NULL is legal IN THESE TWO CALLS ONLY: the bytes are delivered
 * and pos, the exclusive prefix sum of w_var_len, is not (n_rows and n_var are still filled); both
 * pointers NULL stays the sizes-only call.  `narrow` is clg_decode_logs_columns_packed's `out`,
 * `wide` is clg_pack_wide's.  Ranges, flush rules, decode errors and statuses are the existing
 * calls': each span's records up to its first error are packed and the decode's status is
 * returned.  A capacity failure of any output fills every size and writes nothing.  One engine
 * guard covers the whole call; the wide pack's kernel time is the stat "pack_wide". */
int clg_decode_logs_columns_packed_wide(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                                        clg_columns* sizes, clg_payloads* var, clg_packed* narrow, clg_packed_wide* wide);
int clg_decode_host_columns_packed_wide(clg_engine* e, const uint8_t* bytes, const uint64_t* span_off,
                                        const uint64_t* span_len, uint32_t n, clg_columns* sizes, clg_payloads* var,
                                        clg_packed* narrow, clg_packed_wide* wide);

/* ---- replay-prep (DeterminantResponseEvent.merge + LogReplayer decode) ----------------
 * `n` candidate copies of logs (e.g. one per responding GPU / downstream):
 * copy i is (key[i], bytes[off[i], off[i]+len[i])).  For every distinct key the LONGEST
 * copy wins, ties going to the later copy (merge :137-146, v2 on ties).  winner[k] and
 * the number of keys are returned; the winners are then decoded in one batch. */
int clg_replay_prep(clg_engine* e, const uint64_t* key, const uint8_t* bytes, const uint64_t* off,
                    const uint64_t* len, uint32_t n, uint32_t* winner, uint32_t* n_keys,
                    clg_decoded* out, uint64_t* span_rec_base);

/* ---- piggybacked deltas (AbstractDeltaSerializerDeserializer.java:89-163) -----------------
 * enrichWithCausalLogDelta for a batch of outgoing buffers.  Request i covers entries
 * [first, first + count) of log[] / flags[]: the logs the reference's strategy visits for
 * that channel, in its iteration order, after the strategy's pre-hasDelta filters:
 *   CLG_DELTA_FLAT          FlatDeltaSerializerDeserializer.serializeDataStrategy :57-90
 *   CLG_DELTA_HIERARCHICAL  GroupingDeltaSerializerDeserializer.serializeDataStrategy
 *                           :91-165 (vertex-major: the vertex's main log first, then its
 *                           partitions' subpartition logs, each partition contiguous)
 * hasDeltaForConsumer is called on every entry (with its side effects); the delta is sent
 * when it has bytes and the entry's CLG_DE_SEND flag is set (the Grouping strategy's
 * post-hasDelta subpartition filter, :148-151).  Output per request at out_off: the delta
 * header ([size i32][epoch i64] + strategy records, :93-103) then the deltas back to back;
 * out_len = header + deltas.  CLG_E_CAPACITY: *total = required, no consumer moved. */
#define CLG_DELTA_FLAT 0u
#define CLG_DELTA_HIERARCHICAL 1u
#define CLG_DE_SEND 1u

typedef struct clg_enrich_req {
  clg_channel_id consumer;
  int64_t epoch;
  uint32_t first;
  uint32_t count;
  int32_t status;        /* out */
  uint32_t header_bytes; /* out */
  uint64_t out_off;      /* out */
  uint64_t out_len;      /* out */
} clg_enrich_req;

int clg_enrich_batch(clg_engine* e, uint32_t strategy, clg_enrich_req* reqs, uint32_t n, const uint32_t* log,
                     const uint8_t* flags, void* out, uint64_t cap, uint32_t out_kind, uint64_t* total);

/* processCausalLogDelta (:117-163) + insertNewUpstreamLog (:165-194): parse one header +
 * deltas (msg, host or device) and apply processUpstreamDelta to every log it names,
 * opening the logs not seen before (in `job`).  *epoch = the header's epoch; handles[] receives the
 * logs in header order (*n_logs, up to cap); *consumed = header + delta bytes. */
int clg_process_delta(clg_engine* e, uint32_t job, uint32_t strategy, const uint8_t* msg, uint64_t n,
                      uint32_t in_kind, int64_t* epoch, uint32_t* handles, uint32_t cap, uint32_t* n_logs,
                      uint64_t* consumed);

/* ---- batched encode (SimpleDeterminantEncoder.encodeTo :56-75, writers :124-323) ---------
 * The inverse of the decode: records given in the decode's SoA layout (tag, v0; a
 * side-table row per wide record, rows in record order and w_idx naming the record;
 * w_var_off indexes `var`, the payload bytes: TimerTrigger names, storage references,
 * Serializable streams) are written back to back in record order -- exactly the bytes
 * the reference's appendDeterminant sequence would produce.  *n_out = bytes (also on
 * CLG_E_CAPACITY).  A record with tag > 7, a wide record without a side row or whose side
 * row names another record, or a side row whose format carries a payload (a Serializable, a
 * TimerTrigger with sub == 6, a SourceCheckpoint with sub & 0x80) and whose
 * w_var_off + w_var_len passes var_len (64 bits): CLG_E_INVALID_ARG with the lowest such
 * record's index in *bad_index, nothing written.  Rows without a payload do not read
 * w_var_off / w_var_len.  More side rows given than the wide records use: CLG_E_INVALID_ARG
 * with *bad_index == n. */
typedef struct clg_encode_in {
  const uint8_t* tag;
  const int64_t* v0;
  uint64_t n;
  const uint32_t* w_idx;
  const int32_t* w_rc;
  const int64_t* w_v1;
  const uint32_t* w_var_off;
  const uint32_t* w_var_len;
  const uint8_t* w_sub;
  uint64_t n_wide;
  const uint8_t* var;
  uint64_t var_len;
  uint32_t in_kind; /* CLG_MEM_HOST / CLG_MEM_DEVICE (all input arrays) */
  uint32_t reserved;
} clg_encode_in;

int clg_encode_batch(clg_engine* e, const clg_encode_in* in, void* out, uint64_t cap, uint32_t out_kind,
                     uint64_t* n_out, uint64_t* bad_index);

/* ---- encode typed columns --------------------------------------------------
 * The inverse of clg_decode_logs_columns_var: typed columns and their payload column go in, each
 * span's exact log bytes come out.  Record i's bytes are the ones clg_encode_batch writes for the
 * columns' SoA row: its value comes from its class column at its rank in that class; a wide
 * record's rc / v1 / sub / len from wide row k, its rank among the wide tags; its payload is
 * var[pos[k] : pos[k] + w_var_len[k]], read only where the format carries one (a TimerTrigger with
 * sub == 6, a SourceCheckpoint with sub & 0x80, a Serializable).  w_var_off is not an input (it
 * indexes bytes that are not there); w_idx is optional (NULL: not checked).  pos and var may be
 * NULL when no wide row carries a payload.  span_base is host memory, (n_spans + 1) x 5 entries
 * as clg_columns.span_base; NULL with n_spans 0: one span.  in_kind holds for every other array
 * (CLG_MEM_HOST: staged; CLG_MEM_DEVICE; CLG_MEM_MAPPED: registered host memory, read in place). */
typedef struct clg_columns_in {
  const uint8_t* tag;          /* [n_rec] */
  const int8_t* order;         /* [n_class[0]] */
  const int64_t* timestamp;    /* [n_class[1]] */
  const int32_t* rng;          /* [n_class[2]] */
  const int32_t* buffer_built; /* [n_class[3]] */
  const int32_t* w_rc;         /* the wide rows, [n_class[4]] each */
  const int64_t* w_v1;
  const uint32_t* w_var_len;
  const uint8_t* w_sub;
  const int64_t* w_v0;
  const uint32_t* w_idx;       /* optional */
  const uint64_t* pos;         /* [n_class[4] + 1] */
  const uint8_t* var;          /* [n_var] */
  const uint64_t* span_base;   /* host memory */
  uint64_t n_rec;
  uint64_t n_class[CLG_COL_CLASSES];
  uint64_t n_var;
  uint32_t n_spans;
  uint32_t in_kind;
} clg_columns_in;

/* What was wrong with the input (clg_encoded.bad_what); bad_index is always the lowest index of
 * the kind reported.  When several kinds are present the first in this order is reported. */
enum {
  CLG_ENC_BAD_NONE = 0,
  CLG_ENC_BAD_TAG = 1,    /* a tag above 7: the record */
  CLG_ENC_BAD_TOTALS = 2, /* a class's tag count differs from n_class[c]: the class */
  CLG_ENC_BAD_SPAN = 3,   /* span_base rows decrease, the last row is not n_class, or the class
                             counts of the tags before a span's first record are not its row: the span */
  CLG_ENC_BAD_ROW = 4     /* pos[k] + w_var_len[k] > n_var (64 bits) for a row whose format carries
                             a payload, or w_idx[k] is not the k-th wide record: the row */
};
typedef struct clg_encoded {
  void* bytes;              /* NULL: sizes only (n_bytes and span_byte_base are filled) */
  uint64_t cap;
  uint32_t out_kind;        /* CLG_MEM_HOST / CLG_MEM_DEVICE / CLG_MEM_MAPPED */
  uint32_t reserved;
  uint64_t* span_byte_base; /* host memory, n_spans + 1 entries (one span: 2), or NULL: the byte
                               offset of each span's first record; the last entry is n_bytes */
  /* results */
  uint64_t n_bytes;
  uint32_t bad_what;
  uint32_t reserved2;
  uint64_t bad_index;       /* ~0 when none */
} clg_encoded;

/* Invalid input (the kinds above): CLG_E_INVALID_ARG, nothing written.  cap < n_bytes:
 * CLG_E_CAPACITY with n_bytes and span_byte_base filled and nothing written.  CLG_MEM_DEVICE
 * output is written by the kernels; CLG_MEM_HOST and CLG_MEM_MAPPED output goes through engine
 * scratch and one copy.  Synchronous. */
int clg_encode_columns(clg_engine* e, const clg_columns_in* in, clg_encoded* out);
/* The same bytes on the CPU (no engine, no GPU): every array is host memory. */
int clg_encode_columns_host(const clg_columns_in* in, clg_encoded* out);
/* Encode into engine scratch in HBM, then span s becomes one appendDeterminant batch of log[s] in
 * epoch[s], in span order, scattered into the log's segments on the device (no encoded byte
 * crosses the link; the write path's Serializable sidecar is filled as for any other byte).
 * n_spans is in->n_spans (1 when that is 0).  Pending host bytes are flushed first.  status[s]:
 * CLG_OK, CLG_E_NO_LOG, CLG_E_NOSPACE, or CLG_E_INVALID_ARG for a span of 2^31 bytes or more; a
 * failed span leaves its log untouched and the other spans are applied; a depth-0 log is skipped.
 * A log may appear more than once: its spans apply in order.  span_bytes[s] (may be NULL): the
 * span's encoded length.  An invalid `in` fails the whole call before any log changes (the kinds
 * are clg_encode_columns'; the call's error text names them). */
int clg_append_columns(clg_engine* e, const uint32_t* log, const int64_t* epoch, uint32_t n_spans,
                       const clg_columns_in* in, uint64_t* span_bytes, int32_t* status);
/* clg_encode_columns / clg_append_columns with the five narrow columns given packed: `narrow` is
 * unpacked into engine-owned device scratch (kept between calls) and the existing encode runs on
 * it, so no plain narrow column crosses the link.  `rest` carries everything else: its five narrow
 * pointers must be NULL (CLG_E_INVALID_ARG), its n_rec and n_class[0 .. 3] must equal
 * narrow->n_val[0 .. 4] (CLG_UNPACK_BAD_LAYOUT, stream: the lowest that differs); rest->in_kind
 * holds for the wide rows, pos and var, independently of narrow->out_kind.  A bad packed input
 * fails the whole call with CLG_E_INVALID_ARG and `bad` filled (out->bad_what stays 0; every
 * status[s] stays CLG_OK) before anything is written or any log changes.  After a clean unpack
 * the results, errors, per-span statuses and span_bytes are clg_encode_columns' /
 * clg_append_columns' exactly (a tag above 7 is CLG_ENC_BAD_TAG).  One engine guard covers the
 * whole call. */
int clg_encode_columns_packed(clg_engine* e, const clg_packed* narrow, const clg_columns_in* rest,
                              clg_encoded* out, clg_unpack_bad* bad);
int clg_append_columns_packed(clg_engine* e, const uint32_t* log, const int64_t* epoch, uint32_t n_spans,
                              const clg_packed* narrow, const clg_columns_in* rest,
                              uint64_t* span_bytes, int32_t* status, clg_unpack_bad* bad);

/* ---- packed wide rows as input ----------------------------------------------
 * clg_unpack_wide_host on the device: the seven w_* arrays of `out` are written under cap_wide and
 * out->out_kind, n_class[4] is filled, nothing else of `out` is touched.  pos (optional; the same
 * memory kind, 8-byte aligned, cap_wide + 1 entries) receives the exclusive prefix sum of w_var_len
 * as u64, pos[n_wide] the total: the payload column's pos, which the packed-wide decodes do not
 * deliver.  Statuses and their order are clg_unpack_wide_host's exactly: the layout, then the
 * sizes; all seven pointers and pos NULL: sizes only (no descriptor is read); CLG_E_CAPACITY with
 * nothing written; then every block (pos % 16 == 0 included), then every value (a KIND above 3;
 * KIND's histogram, stream 0 block 0, before the other streams' values), each kind of finding
 * with its lowest (stream, block).  Invalid input writes nothing to the caller's arrays, whatever
 * their kind.  Memory rules are clg_unpack_columns': device and registered input is read in place
 * (bits 16-byte, desc 8-byte aligned, else CLG_E_INVALID_ARG), host input is staged with one copy
 * each; device and registered outputs aligned to their element are written by the kernels, host
 * outputs through engine scratch and one copy each.  No byte outside [0, n_wide) of an array or
 * [0, n_wide] of pos is written.  An input without rows launches nothing.  Synchronous; takes the
 * engine guard; the kernels' time is the stat "unpack_wide". */
int clg_unpack_wide(clg_engine* e, const clg_packed_wide* in, clg_columns* out, uint64_t* pos, clg_unpack_bad* bad);

/* clg_encode_columns / clg_append_columns with the narrow columns AND the wide rows given packed:
 * both are unpacked into engine-owned device scratch, pos is rebuilt there, and the existing
 * encode runs on it, so no plain column, wide row or pos exists on the host.  `rest` carries var,
 * n_var, span_base, n_spans, n_rec and n_class[0 .. 4]; its five narrow pointers, five w_*
 * pointers, w_idx and pos must all be NULL (CLG_E_INVALID_ARG); rest->in_kind governs only var.
 * The checks, in order: narrow's layout and totals (as clg_encode_columns_packed); wide's layout
 * (LAYOUT, CLG_UNPACK_WIDE_STREAM + stream); wide->n_val[KIND] != rest->n_class[4] (LAYOUT, stream
 * CLG_UNPACK_WIDE_STREAM, block 0); narrow's block and value findings; wide's, with stream
 * CLG_UNPACK_WIDE_STREAM + c; the cross rule: row k names a wide record of its own kind,
 * tag[w_idx[k]] - 3 == KIND[k] (the lowest offending row: VALUE, stream CLG_UNPACK_WIDE_STREAM +
 * CLG_WPACK_IDX, block k / CLG_PACK_BLOCK); then the encode's own checks, results and per-span
 * statuses, which are clg_encode_columns' / clg_append_columns' exactly (the unpacked w_idx is
 * handed to the encode).  A bad packed input fails the whole call with CLG_E_INVALID_ARG and `bad`
 * filled before any byte of `out` is written or any log changes (out->bad_what stays 0; every
 * status[s] stays CLG_OK).  One engine guard covers the whole call.  The _host call is the same on
 * the CPU (no engine, no GPU; every array host memory). */
#define CLG_UNPACK_WIDE_STREAM 32   /* in the combined calls, a finding in `wide` reports stream 32 + its stream */
int clg_encode_columns_packed_wide(clg_engine* e, const clg_packed* narrow, const clg_packed_wide* wide,
                                   const clg_columns_in* rest, clg_encoded* out, clg_unpack_bad* bad);
int clg_append_columns_packed_wide(clg_engine* e, const uint32_t* log, const int64_t* epoch, uint32_t n_spans,
                                   const clg_packed* narrow, const clg_packed_wide* wide, const clg_columns_in* rest,
                                   uint64_t* span_bytes, int32_t* status, clg_unpack_bad* bad);
int clg_encode_columns_packed_wide_host(const clg_packed* narrow, const clg_packed_wide* wide,
                                        const clg_columns_in* rest, clg_encoded* out, clg_unpack_bad* bad);

/* ---- the packed payload column ---------------------------------------------
 * The payload column (clg_payloads: var, pos) front-coded against same-length anchor rows, so that
 * the repeated names and Java streams cross the link once (clonos_amd/csrc/ppay.h is the format's
 * one definition).  For a column of n_rows rows, len_k = pos[k + 1] - pos[k]:
 *   tile t     rows [1024 t, min(1024 (t + 1), n_rows)), one block of the LCP stream
 *   anchor(k)  the lowest row j of k's tile with len_j == len_k; it depends on the lengths alone,
 *              so nothing about it is stored
 *   lcp_k      0 when anchor(k) == k, else the count of leading bytes in which rows k and anchor(k)
 *              agree, 0 .. len_k (the pack emits the maximum)
 *   tail_k     bytes [lcp_k, len_k) of row k
 * desc and bits hold the stream lcp u32[n_rows], FOR, in clg_packed's block format exactly, one
 * block a tile; tail holds the tails back to back in row order, n_tail bytes.  Row k decodes to
 * tail_anchor(k)[0 : lcp_k] followed by tail_k: every row is packed and unpacked on its own.  The
 * lengths are not stored (the wide rows carry them as w_var_len), so the unpack takes pos.
 * n_tail <= n_var and n_bits is at most that of 1024-value blocks of 32-bit values. */
#define CLG_PPAY_STREAM 64   /* clg_unpack_bad.stream of a finding in a packed payload column */
typedef struct clg_packed_payloads {
  clg_pack_block* desc;
  uint8_t* bits;
  uint8_t* tail;
  uint64_t cap_desc;      /* blocks */
  uint64_t cap_bits;      /* bytes */
  uint64_t cap_tail;      /* bytes */
  uint32_t out_kind;      /* CLG_MEM_HOST / CLG_MEM_DEVICE / CLG_MEM_MAPPED (all three arrays) */
  uint32_t reserved;
  /* results */
  uint64_t n_rows;
  uint64_t n_var;
  uint64_t n_bits;        /* bytes used of bits */
  uint64_t n_tail;        /* bytes used of tail */
  uint64_t bad_row;       /* ~0 when none */
} clg_packed_payloads;

/* Pack the payload column var (pos[n_rows] bytes), pos (n_rows + 1 entries), both under in_kind.
 * The rules are clg_pack_columns': device and registered memory are read and written in place
 * (bits 16-byte aligned, desc and pos 8-byte aligned, else CLG_E_INVALID_ARG), host memory goes
 * through engine staging; all three outputs NULL is the sizes-only call; a capacity below its
 * total is CLG_E_CAPACITY with every result filled and nothing written.  pos[0] != 0, a decreasing
 * pos or a row of 2^32 bytes or more: CLG_E_INVALID_ARG with the lowest such row in bad_row and
 * nothing written; no byte of var outside [0, pos[n_rows]) is read, and none of a tile that holds
 * such a row.  n_rows == 0 launches nothing.  Synchronous; takes the engine guard; the kernels'
 * time is the stat "pack_payloads". */
int clg_pack_payloads(clg_engine* e, const uint8_t* var, const uint64_t* pos, uint64_t n_rows,
                      uint32_t in_kind, clg_packed_payloads* out);
/* The same bytes and rules on the CPU (no engine, no GPU): every array is host memory. */
int clg_pack_payloads_host(const uint8_t* var, const uint64_t* pos, uint64_t n_rows, clg_packed_payloads* out);
/* The way back: out->var is written under cap_var and out->out_kind, n_rows and n_var are filled,
 * out->pos is not touched.  pos (under pos_kind) is the column's pos, as clg_unpack_wide delivers
 * it.  var NULL: sizes only.  cap_var < n_var: CLG_E_CAPACITY with nothing written.  The input is
 * not trusted (in->out_kind names where desc, bits and tail live; the memory rules are
 * clg_unpack_columns').  Findings are reported with stream = CLG_PPAY_STREAM and write nothing, in
 * this order, each with its lowest block (a tile):
 *   LAYOUT  cap_desc below ceil(n_rows / 1024), a capacity below its total, a null array that
 *           would be read (pos among them); block 0; checked on the host before the sizes
 *   BLOCK   clg_unpack_columns' block rules, pos % 16 == 0 included
 *   VALUE   an lcp above its row's length, a non-zero lcp on a row that is its own anchor,
 *           pos[0] != 0, a decreasing pos, a row of 2^32 bytes or more
 *   TOTAL   the sum of len_k - lcp_k differs from n_tail, or pos[n_rows] from in->n_var; block 0
 * Synchronous; takes the engine guard; the kernels' time is the stat "unpack_payloads". */
int clg_unpack_payloads(clg_engine* e, const clg_packed_payloads* in, const uint64_t* pos, uint32_t pos_kind,
                        clg_payloads* out, clg_unpack_bad* bad);
/* The same call on the CPU (no engine, no GPU): every array is host memory. */
int clg_unpack_payloads_host(const clg_packed_payloads* in, const uint64_t* pos, clg_payloads* out, clg_unpack_bad* bad);

/* ---- DeterminantResponseEvent (DeterminantResponseEvent.java:36-148) ---------------------
 * The event's map CausalLogID -> log bytes is held as an entry array in the iteration
 * order of the reference's java.util.HashMap (JDK 8: 2^k buckets from 16, load factor
 * 0.75, bins keep insertion order); `table_cap` is that map's bucket count.  Entries
 * point at caller memory (clg_response_read: into the wire bytes).  A zeroed struct with
 * entries/cap set is an empty map. */
typedef struct clg_response_entry {
  clg_causal_log_id id;
  const uint8_t* bytes;
  uint64_t len;
} clg_response_entry;

typedef struct clg_response {
  int32_t found;
  int16_t vertex_id;
  int16_t reserved;
  int64_t correlation_id;
  uint32_t n;          /* entries, map iteration order */
  uint32_t cap;        /* capacity of `entries` */
  uint32_t table_cap;  /* HashMap bucket count (0: fresh map, 16) */
  uint32_t reserved2;
  clg_response_entry* entries;
} clg_response;

/* HashMap.put (:54-63 constructors, JobCausalLogImpl.java:197-199): insert or replace. */
int clg_response_put(clg_response* r, const clg_causal_log_id* id, const uint8_t* bytes, uint64_t len);
/* n puts in order (one call for a response of many logs, e.g. a cross-GPU merge's winners). */
int clg_response_put_batch(clg_response* r, const clg_causal_log_id* ids, const uint8_t* const* bytes,
                           const uint64_t* lens, uint32_t n);
/* write (:93-107).  *n_out = wire size (also on CLG_E_CAPACITY). */
int clg_response_write(const clg_response* r, uint8_t* out, uint64_t cap, uint64_t* n_out);
/* read (:109-125).  The count byte is signed: 128..255 entries read back as none, like the
 * reference.  *consumed = bytes read.  Truncated input: CLG_E_TRUNCATED. */
int clg_response_read(const uint8_t* in, uint64_t n, clg_response* r, uint64_t* consumed);
/* acc.merge(other) (:128-148): nothing if neither is found; per CausalLogID the longer
 * buffer wins, ties -> other's (v2). */
int clg_response_merge(clg_response* acc, const clg_response* other);
/* CausalLogID.hashCode (:151-163), for callers keeping their own maps. */
int32_t clg_causal_log_id_hash(const clg_causal_log_id* id);

/* ---- replay preparation (ReplayingState.java:58-214, LogReplayerImpl.java:51-158) --------
 * For each failed vertex v: its merged response (WaitingDeterminantsState.java:57,102 --
 * start from found=true and clg_response_merge every response in arrival order) and the
 * task's subpartition table.  One batch on the GPU:
 *   main logs  -- CausalLogID(v) of each vertex (absent: empty span), batched decode into
 *                 `main` (span v; LogReplayerImpl replays that record sequence);
 *   subpartition buffers -- for table entry j the response's log (absent: EMPTY_BUFFER),
 *                 BufferBuilt sizes into buffer_sizes[sizes_base[j] ...]
 *                 (SubpartitionRecoveryThread.run :161-188); sub_status[j] is CLG_OK or the
 *                 error that thread hits first (decode error of the record at sub_err_off,
 *                 or CLG_E_NOT_BUFFER_BUILT); sizes before the error are valid and
 *                 sub_count[j] gives their number.  Entries are global over all vertices, in
 *                 vertex order then table order. */
typedef struct clg_replay_vertex {
  const clg_response* acc;
  const clg_causal_log_id* subpartitions;
  uint32_t n_subpartitions;
  int16_t vertex_id;
  int16_t reserved;
} clg_replay_vertex;

typedef struct clg_replay_out {
  clg_decoded* main;          /* host output (out_kind CLG_MEM_HOST) */
  uint64_t* main_rec_base;    /* n_vertices + 1 */
  int32_t* buffer_sizes;      /* capacity sizes_cap */
  uint64_t sizes_cap;
  uint64_t* sizes_base;       /* n_subpartitions_total + 1 */
  uint64_t* sub_count;
  int32_t* sub_status;
  int64_t* sub_err_off;
  int32_t* sub_err_tag;
} clg_replay_out;

int clg_replay_prepare(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_out* out);
/* The same with every response entry's bytes in device memory on the engine's device (e.g.
 * the winners of a cross-GPU merge in an RCCL receive buffer): they are gathered into the
 * engine's staging area on the GPU, never through the host.  The gather reads whole aligned
 * 16-byte words, so each range needs 16 readable bytes before and after it inside its
 * allocation. */
int clg_replay_prepare_device(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_out* out);

/* Replay preparation that delivers the main logs as typed columns (clg_columns, above) and,
 * with `var`, the wide rows' payload bytes (clg_payloads) -- what a LogReplayerImpl cursor
 * consumes, with no byte offsets into the responses left to resolve.  Lookup, staging, the
 * subpartition kernels and every subpartition output are clg_replay_prepare's; only the
 * main-log step differs.  Status and errors are clg_decode_host_columns_var's: the columns'
 * status wins when it is not CLG_OK; with a decode error each vertex's records up to its first
 * error are delivered and main's error fields are filled; on CLG_E_CAPACITY the totals,
 * main->span_base and the payload sizes are filled and no column is written.  The sizes_cap
 * check comes first, as in clg_replay_prepare; the subpartition outputs are complete whenever
 * the call got past it.  An absent main log is an empty span; n == 0 is valid. */
typedef struct clg_replay_columns_out {
  clg_columns* main;       /* span i = vertex i; main->span_base: (n + 1) * 5 host entries or NULL */
  clg_payloads* var;       /* the wide rows' payloads of `main`; NULL: none */
  int32_t* buffer_sizes;   /* from here on exactly clg_replay_out's subpartition fields */
  uint64_t sizes_cap;
  uint64_t* sizes_base;
  uint64_t* sub_count;
  int32_t* sub_status;
  int64_t* sub_err_off;
  int32_t* sub_err_tag;
} clg_replay_columns_out;
int clg_replay_prepare_columns(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_columns_out* out);
/* ... with every response entry's bytes in device memory (clg_replay_prepare_device's rules). */
int clg_replay_prepare_columns_device(clg_engine* e, const clg_replay_vertex* v, uint32_t n,
                                      clg_replay_columns_out* out);

/* Replay preparation that delivers the main logs as packed typed columns: what a recovering task
 * calls to get the blocks its cursor pops one typed value at a time from.  Lookup, staging, the
 * subpartition kernels and every subpartition output are clg_replay_prepare's; the main step is
 * clg_decode_host_columns_packed over the staged bytes (with `wide`:
 * clg_decode_host_columns_packed_wide), and statuses, decode errors and capacities are that
 * call's: with a decode error each vertex's records up to its first error are packed, the error
 * fields of `sizes` are filled and the decode's status is returned; on CLG_E_CAPACITY every size is
 * filled and nothing is written.  The sizes_cap check comes first; the subpartition outputs are
 * complete whenever the call got past it.  An absent main log is an empty span; n == 0 is valid.
 * A batch within the one-launch limits (at most 69 narrow blocks and 8 193 wide rows) is packed by
 * one kernel launch. */
typedef struct clg_replay_packed_out {
  clg_columns* sizes;      /* totals, span_base ((n + 1) * 5 host entries or NULL), error fields; the narrow
                              pointers NULL; with `wide` every column pointer NULL, else the seven w_* arrays plain */
  clg_payloads* var;       /* the wide rows' payloads; NULL: none; with `wide`, pos may be NULL */
  clg_packed* narrow;      /* the five narrow columns, packed */
  clg_packed_wide* wide;   /* the wide rows, packed; NULL: plain in `sizes` */
  int32_t* buffer_sizes;   /* from here on exactly clg_replay_out's subpartition fields */
  uint64_t sizes_cap;
  uint64_t* sizes_base;
  uint64_t* sub_count;
  int32_t* sub_status;
  int64_t* sub_err_off;
  int32_t* sub_err_tag;
} clg_replay_packed_out;   /* 88 bytes */
int clg_replay_prepare_columns_packed(clg_engine* e, const clg_replay_vertex* v, uint32_t n, clg_replay_packed_out* out);
/* ... with every response entry's bytes in device memory (clg_replay_prepare_device's rules). */
int clg_replay_prepare_columns_packed_device(clg_engine* e, const clg_replay_vertex* v, uint32_t n,
                                             clg_replay_packed_out* out);

/* getDeterminants(start_epoch[i]) of log[i] (:285-313) for n logs -- the copies
 * respondToDeterminantRequest answers with (JobCausalLogImpl.java:188-204) -- gathered by ONE
 * kernel back to back in request order into `out` (host or device); len[i] and out_off[i]
 * (optional) give each copy's size and place.  out == NULL: sizes only (*total = bytes
 * needed); cap < *total: CLG_E_CAPACITY. */
int clg_get_determinants_batch(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                               void* out, uint64_t cap, uint32_t out_kind, uint64_t* out_off, uint32_t* len,
                               uint64_t* total);

/* ---- log digests ------------------------------------------------------------------------------
 * A way to say that two copies of a log hold the same bytes without moving those bytes: 16 bytes
 * per log.  The digest of a span of n bytes b[0..n) is the pair {hash, len = n}, with
 *   p = 2^61 - 1, R = 2654435761 (a primitive root mod p), m = ceil(n / 4),
 *   w_k = the little-endian u32 of bytes 4k .. 4k+3, zero-padded past n,
 *   hash = ( sum_{k<m} w_k * R^(m-1-k) ) mod p, always reduced to [0, p)
 * (h = 0, then h = (h * R + w_k) mod p per word).  Two spans are taken as equal only when BOTH
 * fields are equal.  Differing spans of equal length collide with probability at most m / p:
 * this protects against accidents, not adversaries. */
typedef struct clg_digest {
  uint64_t hash;
  uint64_t len;
} clg_digest;
/* Digest of getDeterminants(start_epoch[i]) of log[i], n logs, one read-only pass over HBM; only
 * n * 16 bytes come back.  The range rules are clg_get_determinants_batch's (depth-0 log and
 * empty range: {0, 0}; unknown handle: CLG_E_NO_LOG; absent epoch: from the earliest), staged
 * appends are flushed first, requests may repeat a log and come in any order.  Strengthens
 * LogReplayerImpl.checkFinished's length-only assertion (LogReplayerImpl.java:126-128): the
 * regenerated log is compared with the recovered one by content. */
int clg_digest_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n, clg_digest* out);
/* Digest of span i = bytes[off[i], off[i]+len[i]) of host or device memory (in_kind CLG_MEM_HOST
 * / CLG_MEM_DEVICE); a span of 2^32 bytes or more is CLG_E_INVALID_ARG.  Device input is read
 * in aligned 16-byte words, only those that hold a byte of a span.  Strengthens
 * DeterminantResponseEvent.merge (DeterminantResponseEvent.java:137-146), which keeps the longer
 * copy on its length alone: the received winner is compared with the log its owner measured. */
int clg_digest_spans(clg_engine* e, const uint8_t* bytes, const uint64_t* off, const uint64_t* len, uint32_t n,
                     uint32_t in_kind, clg_digest* out);
/* The same digest of host bytes on the CPU (no engine, no GPU). */
int clg_digest_host(const uint8_t* bytes, uint64_t n, clg_digest* out);
/* Prefix digests: a range's digest at many cut lengths, the range read once (the hash is a
 * polynomial in R, so the digest of a prefix falls out of the same pass).
 * out[k], cut_first[i] <= k < cut_first[i+1] (cut_first[0] = 0): the digest of the first
 * min(cuts[k], len_i) bytes of getDeterminants(start_epoch[i]) of log[i].  A cut past the end
 * clamps (the row's len then says so), a cut at the end gives clg_digest_logs' row, a cut of 0
 * gives {0, 0}.  Range rules and errors are clg_digest_logs'; cuts of one request must not
 * decrease (CLG_E_INVALID_ARG names the request; nothing is written).  What this lets a caller
 * check: DeterminantResponseEvent.merge (DeterminantResponseEvent.java:137-146) keeps the
 * longest copy of a log and ThreadCausalLogImpl.processUpstreamDelta skips what lies below its
 * own offset, both on the assumption that the shorter copy is a prefix of the longer one; the
 * holder of the longer copy compares its digest at the other side's length with the 16 bytes
 * the other side sent. */
int clg_digest_prefixes(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n,
                        const uint64_t* cut_first, const uint32_t* cuts, clg_digest* out);
/* Cuts at the range's own epoch ends: one row per epoch of the range, in order:
 * epoch_id[k], out[k] = the digest of the range up to the end of that epoch (the last row of a
 * request is clg_digest_logs' row; an empty epoch repeats the row before it; a depth-0 log and
 * a log without epochs have no rows).  first[i]..first[i+1] are request i's rows (n + 1
 * entries); *total rows in all; more than cap: CLG_E_CAPACITY with *total set; out == NULL:
 * sizes only.  Two holders of a log whose rows differ first at epoch E parted in epoch E: the
 * same prefix assumption (DeterminantResponseEvent.java:137-146, ThreadCausalLogImpl's offset
 * dedup) checked epoch by epoch with no log bytes moved. */
int clg_digest_epochs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n, uint64_t cap,
                      uint64_t* first, int64_t* epoch_id, clg_digest* out, uint64_t* total);
/* CPU: the same rows for one span of host bytes, in one pass over it (no engine, no GPU). */
int clg_digest_prefixes_host(const uint8_t* bytes, uint64_t n, const uint32_t* cuts, uint32_t n_cuts, clg_digest* out);

/* ---- log comparison ---------------------------------------------------------------------------
 * Where two copies of a log part, not only whether they do.  lcp is the number of leading bytes
 * the log range and the reference span have in common, lcp <= min(len_log, len_ref):
 *   equal                         lcp == len_log == len_ref
 *   one is a prefix of the other  lcp == min(len_log, len_ref) and the lengths differ
 *   differ                        lcp is the offset of the first differing byte in the range */
typedef struct clg_diff {
  uint64_t lcp;
  uint64_t len_log;
  uint64_t len_ref;
} clg_diff;
/* For each i < n: compare getDeterminants(start_epoch[i]) of log[i] with the reference span
 * bytes[off[i], off[i] + len[i]) of host or device memory (in_kind CLG_MEM_HOST /
 * CLG_MEM_DEVICE), one read-only pass over both where they lie; only n * 24 bytes come back.
 * The range rules are clg_digest_logs' (depth-0 log and empty range: len_log 0; unknown handle:
 * CLG_E_NO_LOG; absent epoch: from the earliest), staged appends are flushed first, requests
 * may repeat a log and come in any order.  A reference span of 2^32 bytes or more is
 * CLG_E_INVALID_ARG.  Host input is staged as clg_digest_spans stages it.  Device input is read
 * in aligned 16-byte words, only those that hold a byte of a span (and of a span only the
 * first min(len_log, len_ref) bytes): the caller's buffer need not be padded or aligned.
 * After a failed length check (LogReplayerImpl.checkFinished, LogReplayerImpl.java:126-128) or
 * a failed digest comparison this names the byte at which the regenerated log left the
 * recovered one; and where DeterminantResponseEvent.merge (DeterminantResponseEvent.java:137-146)
 * keeps the longer copy on its length alone, it says whether the shorter one is a prefix of it
 * (a copy that lags) or not (a corrupt one). */
int clg_diff_logs(clg_engine* e, const uint32_t* log, const int64_t* start_epoch, uint32_t n, const uint8_t* bytes,
                  const uint64_t* off, const uint64_t* len, uint32_t in_kind, clg_diff* out);
/* The same of two host byte strings on the CPU (no engine, no GPU). */
int clg_lcp_host(const uint8_t* a, uint64_t na, const uint8_t* b, uint64_t nb, uint64_t* lcp);

/* ---- in-flight (data) log (RT/inflightlogging/, I/ below) -------------------------------------
 * InFlightLog I/InFlightLog.java:32-55, two implementations (I/InFlightLogConfig.java:44 picks
 * one by taskmanager.inflight.type, default "spillable"):
 *   CLG_IFL_IN_MEMORY  InMemorySubpartitionInFlightLogger I/InMemorySubpartitionInFlightLogger.java:28-207
 *   CLG_IFL_SPILLABLE  SpillableSubpartitionInFlightLogger I/SpillableSubpartitionInFlightLogger.java:45-341
 *                      with SpilledReplayIterator I/SpilledReplayIterator.java:60-401 (replay semantics;
 *                      the spill files are not modelled -- every buffer stays in HBM, i.e. no spill
 *                      has completed, which is the deterministic case of the reference)
 * Per subpartition, the data buffers sent in each epoch, kept in HBM (the engine's in-flight pool,
 * clg_config.ifl_*; a buffer spans ceil(len / ifl_segment_bytes) segments) until a checkpoint
 * completes.  The Java side keeps refcounts; the engine owns the bytes.  A full pool is
 * CLG_E_NOSPACE with nothing logged: the caller applies backpressure (waits for a checkpoint to
 * free epochs) and retries. */
#define CLG_IFL_IN_MEMORY 0u
#define CLG_IFL_SPILLABLE 1u
int clg_ifl_open(clg_engine* e, uint32_t* handle); /* CLG_IFL_IN_MEMORY */
int clg_ifl_open_typed(clg_engine* e, uint32_t type, uint32_t* handle);
/* close() (in-memory :90-94, spillable :151-157): all buffers released. */
int clg_ifl_close(clg_engine* e, uint32_t ifl);
/* log(buffer, epochID, isFinished) (in-memory :44-48, spillable :84-103), batched: buffer i =
 * bytes[off[i], off[i] + len[i]) appended to ifl[i] in epoch[i], in order (host or device input).
 * Spillable: a buffer logged while the log is replaying (between getInFlightIterator and the
 * drain of its last buffer) reaches the live iterator (notifyNewBufferAdded,
 * SpilledReplayIterator.java:262-277).  When the log is replaying but getInFlightIterator has
 * never returned an iterator (its first call found nothing, :132-135), the reference's log()
 * throws a NullPointerException after appending (:98-99): every buffer is appended and the
 * status is CLG_E_STATE. */
int clg_ifl_log_batch(clg_engine* e, const uint32_t* ifl, const int64_t* epoch, const uint64_t* off,
                      const uint32_t* len, uint32_t n, const uint8_t* bytes, uint32_t in_kind);
/* notifyCheckpointComplete (in-memory :51-70, spillable :106-123): epochs < checkpoint_id are
 * dropped, their segments freed. */
int clg_ifl_notify_checkpoint_complete(clg_engine* e, uint32_t ifl, int64_t checkpoint_id);
/* Epochs and buffer counts (ascending epoch), for parity tests. */
int clg_ifl_state(clg_engine* e, uint32_t ifl, int64_t* epoch_ids, uint32_t* n_buffers, uint32_t cap,
                  uint32_t* n_epochs);
/* getInFlightIterator(startEpochID, ignoreBuffers) + draining the iterator, batched: for request
 * i the buffers the iterator yields after skipping ignore_buffers are gathered by one kernel,
 * back to back in request order, into `out` at out_off (len bytes); their sizes go to
 * sizes[sizes_off ...] (n_buffers entries).  remaining = the iterator's numberRemaining() after
 * the skip.  epochs (optional, indexed like sizes) receives each buffer's epoch: the iterator's
 * getEpoch() right before the next() that returns it, which
 * PipelinedSubpartition.getReplayedBufferUnsafe (:306-320) stamps on the BufferAndBacklog;
 * end_epoch is getEpoch() after the last buffer was taken (or after the skip when none is).
 * CLG_E_CAPACITY (bytes or sizes): *total / *total_buffers hold the required sizes, no bytes are
 * gathered and no iterator state changes.
 *
 * In-memory (ReplayIterator :107-201): the buffers of every epoch >= start when start itself holds
 * buffers, else nothing (:121-127: a start epoch that is absent, e.g. already truncated, yields
 * nothing).  An epoch without buffers between start and the last epoch (K buffers before it):
 * next() advances past each returned buffer (:156) and throws at the gap (:133), so the K-th
 * buffer is never delivered -- buffers [ignore_buffers, K-1) are gathered and status is
 * CLG_E_EPOCH_GAP.  A skip that throws inside getInFlightIterator (:78-79) -- ignore_buffers >= K
 * at a gap, beyond the buffers available without one, or any skip when start is absent -- is
 * CLG_E_STATE, nothing gathered.
 *
 * Spillable (getInFlightIterator :126-142, SpilledReplayIterator, EpochCursor :306-394): the
 * iterator covers tailMap(start) -- the epochs >= start, from the first one present.  Empty (or a
 * closed log): no iterator (res.flags CLG_IFL_NULL_ITERATOR, nothing gathered).  Its cursors step
 * epoch IDs one by one, so an epoch missing between the first and the last makes the iterator
 * throw: a skip reaching past it is CLG_E_STATE (inside the constructor); otherwise the prefetch
 * cursor stops at it in the constructor and the consumer's first next() throws (no buffer is
 * delivered, CLG_E_EPOCH_GAP).  The iterator stays the log's current one: max_buffers (0: all)
 * bounds how many are taken per request, and a request with CLG_IFL_CONTINUE takes the next
 * buffers of the current iterator (start and ignore_buffers unused), including buffers logged
 * since.  Taking its last buffer ends the replay (res.flags loses CLG_IFL_REPLAYING).
 * max_buffers and CLG_IFL_CONTINUE are spillable-only (CLG_E_INVALID_ARG otherwise). */
#define CLG_IFL_CONTINUE 1u       /* clg_ifl_replay_req.flags: continue the current iterator */
#define CLG_IFL_NULL_ITERATOR 1u  /* clg_ifl_replay_res.flags: getInFlightIterator returned null */
#define CLG_IFL_REPLAYING 2u      /* clg_ifl_replay_res.flags: the log is replaying after the call */
typedef struct clg_ifl_replay_req {
  uint32_t ifl;
  uint32_t ignore_buffers;
  int64_t start_epoch;
  uint32_t max_buffers; /* spillable: at most this many buffers taken (0: all) */
  uint32_t flags;       /* CLG_IFL_CONTINUE */
} clg_ifl_replay_req;
typedef struct clg_ifl_replay_res {
  int32_t status;
  uint32_t n_buffers;
  uint32_t remaining;
  uint32_t flags; /* CLG_IFL_NULL_ITERATOR | CLG_IFL_REPLAYING */
  uint64_t out_off;
  uint64_t len;
  uint64_t sizes_off;
  int64_t end_epoch;
} clg_ifl_replay_res;
int clg_ifl_replay_batch(clg_engine* e, const clg_ifl_replay_req* reqs, uint32_t n, clg_ifl_replay_res* res,
                         void* out, uint64_t cap, uint32_t out_kind, uint32_t* sizes, int64_t* epochs,
                         uint64_t sizes_cap, uint64_t* total, uint64_t* total_buffers);

/* ---- instrumentation ---------------------------------------------------------------- */
typedef struct clg_kernel_stat {
  char name[32];
  uint64_t launches;
  double total_ms;
  uint64_t bytes; /* algorithmic bytes attributed to the kernel */
} clg_kernel_stat;
int clg_kernel_stats(clg_engine* e, clg_kernel_stat* out, uint32_t cap, uint32_t* n);
int clg_kernel_stats_reset(clg_engine* e);

#ifdef __cplusplus
}
#endif
#endif /* CLONOS_ENGINE_H */
