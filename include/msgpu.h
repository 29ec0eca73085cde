/*
 * msgpu.h -- C-ABI of the MI355X-native overlap-and-consensus core for MuCHSALSA (libmsgpu.so).
 *
 * Drop-in boundary for the reference's hot path.  Plain C, opaque contexts, caller-owned input buffers,
 * int status codes (0 = ok) + msgpu_*_last_error(); no exception crosses it.  Each entry point names the
 * reference interface it replaces (paths relative to the reference tree).
 *
 *   reference call site (src/main.cpp)                   replaced by
 *   ---------------------------------------------------  --------------------------------------------
 *   ThreadPool(threadCount)                      :143    msgpu_create          (HIP stream dispatcher)
 *   BlastFileAccessor + BlastFileReader::read()  :153-156 msgpu_parse_paf + msgpu_load_rows
 *   MatchMap::calculateEdges()                   :157    msgpu_calculate_edges
 *   SequenceAccessor + buildIndex()              :161-163 msgpu_seq_parse + msgpu_seq_upload (+ msgpu_seq_pack)
 *   for edge: Job(chainingAndOverlaps)           :170-178 msgpu_chaining_and_overlaps
 *   for edge: Job(findContractionEdges)          :183-190 msgpu_find_contraction_edges
 *   contraction ... decycle                      :194-288 msgpu_graph_create + msgpu_graph_clean_up
 *   getConnectedComponents + assemblePaths       :300-310, 620-661  msgpu_graph_linearize + msgpu_graph_path_input
 *   assemblePath per path + OutputWriter         :663-677 msgpu_assembly_add_paths + msgpu_assembly_finish / _text
 *   graph.getEdges()/Edge::getEdgeOrders()/...           msgpu_get_counts + msgpu_copy_tables
 *
 * Semantics are the single-thread reference's, bit for bit: int32 coordinates, IEEE fp64 scores/offsets
 * evaluated in the reference's expression order (kernels are built with -ffp-contract=off).
 */
#ifndef MSGPU_H
#define MSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSGPU_VERSION 1

/* ---- status codes ------------------------------------------------------------------------------------------- */
#define MSGPU_OK 0
#define MSGPU_E_IO (-1)       /* "Can't open blast file."   BlastFileAccessor.cpp:43-45                        */
#define MSGPU_E_FORMAT (-2)   /* "Invalid BLAST file."      BlastFileReader.cpp:97-99                          */
#define MSGPU_E_NUMBER (-3)   /* a field std::stoi would reject (BlastFileReader.cpp:101-116)                  */
#define MSGPU_E_NOMEM (-4)
#define MSGPU_E_ARG (-5)      /* "Unexpected nullptr." & friends (MatchMap.cpp:55-57)                          */
#define MSGPU_E_HIP (-6)      /* a HIP runtime call failed; text in msgpu_last_error                           */
#define MSGPU_E_STATE (-7)    /* entry points called out of order                                              */
#define MSGPU_E_IDS (-8)      /* read ids are not in first-line (Registry) order, Registry.cpp:36-45           */
#define MSGPU_E_NODEVICE (-9) /* no HIP device: the product has NO CPU fallback                                */
#define MSGPU_E_LAYOUT (-10)  /* assemblePath input the reference itself cannot assemble (it would terminate, hang
                                 or read past a container): text in msgpu_assembly_last_error                     */
#define MSGPU_E_TIMEOUT (-11) /* a deadline (msgpu_set_deadline, msgpu_group_set_timeout) passed with device work
                                 still queued: the reference's one catch at src/main.cpp:313-315 sees an error
                                 instead of a process that never returns                                          */

/* ---- records (byte-identical to oracle/ms_oracle.h) ----------------------------------------------------------- */

/* One ACCEPTED PAF line = what BlastFileReader::parseLine hands to Graph::addVertex and
 * MatchMap::addVertexMatch (BlastFileReader.cpp:101-126).  40 bytes. */
typedef struct msgpu_row {
  uint32_t anchor_id; /* illumina/unitig id, Registry first-seen order (registered second, :111)             */
  uint32_t read_id;   /* nanopore id, Registry first-seen order (registered first, :110)                     */
  int32_t  read_len;  /* col 6                                                                                */
  int32_t  i_lo, i_hi; /* VertexMatch::illuminaRange = (col2, col3-1)                                          */
  int32_t  n_lo, n_hi; /* VertexMatch::nanoporeRange = (col7, col8-1)                                          */
  uint32_t score;     /* VertexMatch::score = col 9                                                           */
  uint32_t line;      /* VertexMatch::lineNumber                                                              */
  uint32_t flags;     /* bit0 VertexMatch::direction, bit1 VertexMatch::isPrimary                             */
} msgpu_row;
#define MSGPU_ROW_DIR 1u
#define MSGPU_ROW_PRIMARY 2u

/* The same table as it crosses the host link: 28 bytes per row instead of 40.  What a loader-produced table carries that the
 * link need not (BlastFileReader.cpp:101-126 is what a row must hold): `read_len` once per READ instead of once per row (the
 * Vertex takes it from the read's first line, Graph.cpp:148); `line` as RUNS -- accepted lines are consecutive file lines
 * except where a line was rejected, so line = row index + a delta that changes at few places; the two flag bits in the top
 * bits of the score (a score of 2^30 or more does not pack: msgpu_pack_rows says so and the caller keeps the 40-byte form).
 * msgpu_load_rows_packed expands it in HBM (one kernel, ~0.1 ms for 5 M rows) to exactly the rows msgpu_load_rows would have
 * been given: every table downstream is the same, bit for bit. */
typedef struct msgpu_row28 {
  uint32_t anchor_id, read_id;
  int32_t  i_lo, i_hi, n_lo, n_hi;
  uint32_t score_flags; /* score | direction << 30 | isPrimary << 31 */
} msgpu_row28;
typedef struct msgpu_packed_rows {
  const msgpu_row28 *rows;      /* n_rows of them, in the order of the msgpu_row table                                  */
  uint64_t           n_rows;
  const int32_t     *read_len;  /* n_reads entries: msgpu_row::read_len of the read's FIRST row                         */
  uint32_t           n_reads, n_runs;
  const uint32_t    *run_start; /* n_runs ascending row indices, run_start[0] = 0: rows [run_start[k], run_start[k+1])  */
  const uint32_t    *run_delta; /* ... have line = row index + run_delta[k]                                             */
  void              *owner;     /* msgpu_pack_rows: the one page-locked block everything above lives in                 */
} msgpu_packed_rows;
/* Host code (a few threads): the packed form of a row table whose read ids are < n_reads.  Page-locked memory, to be given
 * back with msgpu_packed_rows_free.  MSGPU_E_ARG when the table does not pack (a score >= 2^30, a read id >= n_reads, a line
 * below its row index -- lines ascend with the rows in a loader's table) -- the 40-byte form takes every input. */
int  msgpu_pack_rows(const msgpu_row *rows, size_t n_rows, uint32_t n_reads, msgpu_packed_rows *out);
void msgpu_packed_rows_free(msgpu_packed_rows *p);

/* graph::Edge (Edge.h:212-218) as a table row.  32 bytes.  Table order: ascending (v1, v2). */
typedef struct msgpu_edge {
  uint32_t v1, v2;    /* Edge::getVertices(): v1 = read with the lower first line (MatchMap.cpp:204-213)      */
  uint64_t em_off;    /* this edge's EdgeMatches are ems[em_off .. em_off+em_cnt)                             */
  uint64_t order_off; /* this edge's EdgeOrders are orders[order_off .. order_off+order_cnt)                  */
  uint32_t em_cnt;
  uint16_t order_cnt;
  uint8_t  shadow;    /* Edge::isShadow (src/main.cpp:389-395)                                                */
  uint8_t  pad;
} msgpu_edge;

/* matching::EdgeMatch (MatchMap.h:68-74).  32 bytes.  Within an edge: ascending
 * (nanoporeRange on v1, anchor_id) = the vStart order of mpp.cpp:164-172. */
typedef struct msgpu_edgematch {
  int32_t  ov_lo, ov_hi; /* EdgeMatch::overlap                                                                */
  double   score;        /* EdgeMatch::score (MatchMap.cpp:200-202)                                           */
  uint32_t anchor_id;
  uint32_t line;         /* EdgeMatch::lineNumber = outerMatch->lineNumber (MatchMap.cpp:218)                 */
  uint32_t flags;        /* bit0 direction, bit1 isPrimary                                                    */
  uint32_t edge_idx;
} msgpu_edgematch;

/* graph::EdgeOrder (Edge.h:49-60).  64 bytes.  Within an edge: emission order of src/main.cpp:397-411
 * (minus-direction paths first, then plus). */
typedef struct msgpu_order {
  uint32_t edge_idx;
  uint32_t flags;        /* MSGPU_ORD_* */
  double   left_offset;
  double   right_offset;
  uint64_t score;        /* path score truncated like path_t's std::size_t (mpp.cpp:34,221,244)               */
  uint64_t ids_off;      /* EdgeOrder::ids = ids[ids_off .. ids_off+ids_cnt)                                  */
  uint32_t ids_cnt;
  uint32_t start, end, base; /* startVertex / endVertex / baseVertex as read ids                              */
  uint32_t pad[2];
} msgpu_order;
#define MSGPU_ORD_START_V1 1u  /* startVertex == v1 (else startVertex == v2, endVertex == v1)                 */
#define MSGPU_ORD_CONTAINED 2u /* EdgeOrder::isContained                                                      */
#define MSGPU_ORD_DIR 4u       /* EdgeOrder::direction                                                        */
#define MSGPU_ORD_PRIMARY 8u   /* EdgeOrder::isPrimary                                                        */

/* compile-time constants of the reference, exposed as parameters ("Config / flags") */
typedef struct msgpu_params {
  uint32_t min_matches; /* 400  MINIMUM_MATCHES  BlastFileReader.cpp:48 */
  uint32_t th_length;   /* 500  TH_LENGTH        BlastFileReader.cpp:49 */
  uint32_t th_matches;  /* 500  TH_MATCHES       BlastFileReader.cpp:50 */
  uint32_t th_overlap;  /* 100  TH_OVERLAP       MatchMap.cpp:41        */
  uint64_t wiggle_room; /* 300  Application::getWiggleRoom, Application.h:132 */
  double   ratio_pct;   /* 15   mpp.cpp:136 */
  double   alt_frac;    /* 0.75 mpp.cpp:223 */
} msgpu_params;

typedef struct msgpu_counts {
  uint64_t n_rows_in;    /* rows handed to msgpu_load_rows                                                    */
  uint64_t n_rows_alive; /* after the (read, anchor) lowest-line rule of MatchMap::addVertexMatch             */
  uint32_t n_reads;      /* Graph::getOrder()                                                                 */
  uint32_t n_anchors;    /* anchor id space                                                                   */
  uint64_t n_edges;      /* Graph::getSize() (this shard)                                                     */
  uint64_t n_ems;        /* EdgeMatches (this shard)                                                          */
  uint64_t n_orders;     /* EdgeOrders (this shard)                                                           */
  uint64_t n_ids;        /* sum of |EdgeOrder::ids| (this shard)                                              */
  uint64_t n_pairs_scanned; /* scaffold rows visited while looking for pairs (both directions of each pair)   */
  uint64_t n_edges_fastpath; /* edges whose pairs were all proven compatible without the O(n^2) sweep (this shard) */
  uint64_t n_lost_publications; /* size read-backs of this context whose publication into mapped host memory never arrived
                                   although the stream finished (the values were re-read by copy): 0 on a healthy system */
  uint64_t index_path;   /* how the last msgpu_load_rows built its index: MSGPU_INDEX_* (same tables whichever way)    */
} msgpu_counts;
#define MSGPU_INDEX_BIN 0u      /* rows binned by coarse read-id bucket, no global atomic per row: rows grouped by anchor with
                                   ascending lines and no duplicate (read, anchor) pair -- what msgpu_parse_paf produces      */
#define MSGPU_INDEX_ATOMIC 1u   /* one counter atomic per row, fixed-size bucket per read (rounds 1-3; MSGPU_NO_BIN=1 forces it) */
#define MSGPU_INDEX_TWO_PASS 2u /* count, scan, scatter: a read with more rows than a fixed bucket holds                      */
#define MSGPU_INDEX_GENERIC 4u  /* OR-ed in: scaffolds built by the generic per-anchor pass (any row order, duplicates)        */

/* Device time of the last run of each stage, milliseconds, measured with HIP events on the context's stream. */
typedef struct msgpu_timings {
  float index_ms;      /* msgpu_load_rows: MatchMap-equivalent index build (device part)                      */
  float candidates_ms; /* msgpu_calculate_edges: pair scan + group by edge                                    */
  float chain_ms;      /* msgpu_chaining_and_overlaps: EdgeMatch + chaining DP + overlap kernel (dominant)    */
  float compact_ms;    /* msgpu_chaining_and_overlaps: order/id compaction                                    */
  float chain_kernel_ms; /* the chain kernels alone (HIP events directly around their launches): mean over the   */
  uint32_t chain_kernel_launches; /* ... msgpu_chaining_and_overlaps calls since the last msgpu_get_timings (<= 256)    */
  uint32_t pad;
} msgpu_timings;

typedef struct msgpu_ctx msgpu_ctx;
typedef struct msgpu_paf msgpu_paf;

/* ---- life cycle ------------------------------------------------------------------------------------------------ */

void msgpu_default_params(msgpu_params *p);
const char *msgpu_strerror(int code);

/* Replaces ThreadPool(threadCount) + Graph + MatchMap construction (src/main.cpp:143-148).
 * `device` is a HIP device ordinal.  Fails with MSGPU_E_NODEVICE when there is none: there is no CPU path. */
int  msgpu_create(int device, const msgpu_params *params, msgpu_ctx **out);
void msgpu_destroy(msgpu_ctx *ctx);
const char *msgpu_last_error(const msgpu_ctx *ctx);

/* ---- STREAM AND THREAD CONTRACT -- who orders what at this boundary ---------------------------------------------------
 * (The reference states its notification contract where it has one: MatchMap observes the Graph's deletions,
 * include/ms/matching/MatchMap.h:200-207.  This boundary's equivalent is stream order.)
 *
 * 1. A context queues all its work on ONE stream: its own (created hipStreamNonBlocking: it does NOT synchronise with the
 *    legacy default stream, nor with any other stream, e.g. the one a tensor library fills buffers on) or the one given to
 *    msgpu_set_stream.  Entry points that take a `hip_stream` argument queue on that stream instead (NULL = the context's).
 * 2. HOST buffers (msgpu_load_rows, msgpu_copy_tables, msgpu_copy_reads, msgpu_find_contraction_edges' result,
 *    msgpu_overlap_batched[_ex], msgpu_get_edgematches): the call returns when the bytes are there / have been consumed.
 *    Nothing to order.
 * 3. DEVICE buffers of the caller -- read: msgpu_load_rows_device (d_rows, until the next load or msgpu_destroy),
 *    msgpu_overlap_batched_ex with MSGPU_BATCH_ROWS_ON_DEVICE, msgpu_merge_gathered[_ex] / msgpu_merge_wire (d_gathered),
 *    msgpu_find_contraction_edges (d_edges, d_orders); written: msgpu_copy_tables_device, msgpu_pack_wire,
 *    msgpu_merge_gathered[_ex] / msgpu_merge_wire (d_edges, d_orders, d_ids) -- are touched ASYNCHRONOUSLY, in the order of
 *    the stream of rule 1 and in no order with anything else.  The CALLER must therefore
 *      (a) have finished -- in stream order -- whatever it queued on those buffers before the call (a fill, a memset, the
 *          all-gather that produced d_gathered): otherwise the library's kernel and the caller's run concurrently and the
 *          buffer ends up a mixture of both;
 *      (b) not read, overwrite or free them before the library's work has finished -- in stream order.
 *    Three ways to meet (a) and (b), cheapest first:
 *      - msgpu_set_stream(ctx, the stream the caller works on): everything is one stream's order;
 *      - msgpu_stream_wait(ctx, s) before the call -- the context's stream waits for what is queued on s so far -- and
 *        msgpu_stream_release(ctx, s) after it -- s waits for what the context has queued so far (two event operations,
 *        no host wait);
 *      - a host wait: the caller synchronises its stream before the call and calls msgpu_synchronize(ctx) after it.
 *    A sequence store (msgpu_seqctx, below) is a context of its own with a stream of its own, and the same rule holds for
 *    the caller's device buffers it touches: msgpu_seq_upload_device (d_bases, read), msgpu_gather_run (d_out, written),
 *    msgpu_fasta_format (d_raw read, d_text written), msgpu_edit_distance (d_a, d_b read); its entry points take the stream to
 *    queue on as `hip_stream` (NULL = the store's own), msgpu_seq_synchronize is its host wait.
 * 4. msgpu_last_error is meaningful only after a call returned a non-zero code.
 * 5. A context is NOT thread-safe: one host thread at a time.  One exception, what an exchange thread needs:
 *    msgpu_merge_gathered_ex / msgpu_merge_wire with a hip_stream of the caller's may run on a second thread beside any
 *    other call (they touch no state of the context except, on failure, the error text). */

/* Run all work of this context on an existing HIP stream (hipStream_t), e.g. the caller's current stream.
 * NULL restores the context's own stream.  Waits for the stream used so far. */
int msgpu_set_stream(msgpu_ctx *ctx, void *hip_stream);
/* The hipStream_t the context queues on at the moment (its own unless msgpu_set_stream changed it). */
void *msgpu_get_stream(const msgpu_ctx *ctx);
/* Rule 3: the context's stream waits for everything queued so far on `hip_stream` (NULL = the legacy default stream);
 * `hip_stream` waits for everything the context has queued so far.  Neither blocks the host. */
int msgpu_stream_wait(msgpu_ctx *ctx, void *hip_stream);
int msgpu_stream_release(msgpu_ctx *ctx, void *hip_stream);

/* Multi-GPU: this context owns the edges whose v1 satisfies v1 % n_shards == shard (default 0 of 1).
 * Every shard loads the full row table; edges/orders of different shards are disjoint and their union is the
 * 1-GPU result.  Must be called before msgpu_calculate_edges. */
int msgpu_set_shard(msgpu_ctx *ctx, uint32_t shard, uint32_t n_shards);

/* Optional: declare the id spaces of the rows that will be loaded (n_reads = highest read id + 1, n_anchors likewise;
 * msgpu_paf_read_count / msgpu_paf_anchor_count of the loader, i.e. Registry::m_ui32Size, Registry.cpp:36-45).  The
 * index build then skips its own pass over the table and one read-back.  Stays in force for later loads; (0, 0)
 * returns to discovery.  A row with an id outside the declared space makes the load fail with MSGPU_E_IDS. */
int msgpu_set_id_space(msgpu_ctx *ctx, uint32_t n_reads, uint32_t n_anchors);

/* ---- A1: PAF loader (host) ------------------------------------------------------------------------------------- */

/* Replaces BlastFileAccessor::_buildIndex (BlastFileAccessor.cpp:77-91) + BlastFileReader::read/parseLine
 * (BlastFileReader.cpp:72-130): indexes all lines, parses all but the LAST one (:76), keeps a line iff
 * col9 >= min_matches and col3-col2 >= min_matches, assigns Registry ids in first-seen order. */
int  msgpu_parse_paf(const char *path, const msgpu_params *params, msgpu_paf **out);
void msgpu_paf_free(msgpu_paf *paf);
const msgpu_row *msgpu_paf_rows(const msgpu_paf *paf, size_t *n_rows);
size_t      msgpu_paf_line_count(const msgpu_paf *paf);
uint32_t    msgpu_paf_read_count(const msgpu_paf *paf);
uint32_t    msgpu_paf_anchor_count(const msgpu_paf *paf);
const char *msgpu_paf_read_name(const msgpu_paf *paf, uint32_t read_id);     /* Registry reverse lookup */
const char *msgpu_paf_anchor_name(const msgpu_paf *paf, uint32_t anchor_id);

/* Registry::operator[] for every record of a parsed sequence file, on the registries of `paf` (the reference's
 * SequenceAccessor calls the very Registry objects BlastFileReader filled: SequenceAccessor.cpp:171,215, src/main.cpp:
 * 149-163): a name the PAF registered keeps its id, an unknown name takes the next free id in file order (the registry
 * grows).  kind 0 = reads (nanopore registry), 1 = unitigs (illumina registry).  ids: msgpu_seq_count(f) entries, what
 * msgpu_seq_upload takes; *id_space (optional) = the registry's size afterwards. */
struct msgpu_seqfile;
int msgpu_paf_register_sequences(msgpu_paf *paf, int kind, const struct msgpu_seqfile *f, uint32_t *ids, uint32_t *id_space);

/* Host utilities of libms that the loader is made of, on their own (the reference's unit tests hold vectors for them:
 * libms/tests/IO_test.cpp:12-35, Registry_test.cpp:5-14, Toggle_test.cpp:5-25; replayed from tests/golden/ref_tests/).
 * msgpu_index_lines: the line index of BlastFileAccessor::_buildIndex (BlastFileAccessor.cpp:77-91) over readline
 * (IO.cpp:54-97): every '\n' ends a line and belongs to it, a non-empty tail without '\n' is a line.  offsets (capacity
 * entries, may be NULL with capacity 0 to count) receives the start of every line and, if it fits, the file size after
 * the last one.  msgpu_registry_*: Registry (Registry.cpp:36-52), dense ids in first-seen order; clear() restarts at 0.
 * msgpu_toggle_mul: Toggle::operator* (Toggle.h:127-153) = XNOR. */
int msgpu_index_lines(const char *path, uint64_t *offsets, size_t capacity, size_t *n_lines);
typedef struct msgpu_registry msgpu_registry;
msgpu_registry *msgpu_registry_new(void);
void     msgpu_registry_free(msgpu_registry *r);
uint32_t msgpu_registry_id(msgpu_registry *r, const char *name); /* operator[]; 0xffffffff on error */
uint32_t msgpu_registry_size(const msgpu_registry *r);
void     msgpu_registry_clear(msgpu_registry *r);
int      msgpu_toggle_mul(int a, int b);

/* ---- A1 tail: fill the device-resident MatchMap/Graph-vertex equivalent ---------------------------------------- */

/* Replaces the effect of BlastFileReader::read() on Graph (addVertex: first line wins, Graph.cpp:148) and
 * MatchMap (addVertexMatch: lowest line per (read, anchor) wins, MatchMap.cpp:52-81).
 * `rows` may be in any order and may contain (read, anchor) duplicates.  Read ids must follow first-line
 * order (what msgpu_parse_paf produces), else MSGPU_E_IDS.  Host buffer; copied to HBM. */
int msgpu_load_rows(msgpu_ctx *ctx, const msgpu_row *rows, size_t n_rows);
/* msgpu_load_rows for the 28-byte form: packed rows over the link (page-locked: msgpu_pack_rows), expanded in HBM. */
int msgpu_load_rows_packed(msgpu_ctx *ctx, const msgpu_packed_rows *packed);
/* Same, rows already resident in HBM (device pointer, n_rows * 40 bytes).  The buffer is only read -- by this call and by
 * every later stage until the next load (STREAM CONTRACT rule 3: the rows must be complete in the context's stream order). */
int msgpu_load_rows_device(msgpu_ctx *ctx, const void *d_rows, size_t n_rows);

/* ---- A2/A3: MatchMap::calculateEdges (MatchMap.cpp:161-224) ----------------------------------------------------- */

/* All pairs of reads sharing an anchor, overlap test (> th_overlap), grouping by edge.  After it returns
 * msgpu_get_counts().n_edges / .n_ems are valid (Graph::getSize()). */
int msgpu_calculate_edges(msgpu_ctx *ctx);

/* ---- A4..A7: the chainingAndOverlaps fan-out (src/main.cpp:170-178, 328-414) ------------------------------------ */

/* EdgeMatch scores, getMaxPairwisePaths (mpp.cpp:145-305) for both directions, the primary/multi filters,
 * Edge::setShadow, getOverlap (ol.cpp:53-101), Edge::appendOrder -- for every edge of this shard. */
int msgpu_chaining_and_overlaps(msgpu_ctx *ctx);

/* ---- results ----------------------------------------------------------------------------------------------------- */

int msgpu_get_counts(msgpu_ctx *ctx, msgpu_counts *out);
int msgpu_get_timings(msgpu_ctx *ctx, msgpu_timings *out);
/* The chain stage's banded pair sweep: edges of more than msgpu_chain_band_width() + 1 EdgeMatches in
 * a kernel that has the band are swept over the pairs (k, l), l - B <= k < l, first, and over all pairs again only when the
 * band's result is not provably the full one.  n_banded: edges of the context's LAST chaining pass that started on the band;
 * n_fallback: those of them that were done again.  Both 0 under MSGPU_NO_BAND=1 / MSGPU_NO_FASTPATH=1.  Read from the device
 * on demand (synchronises the context's stream); not part of msgpu_counts. */
int msgpu_get_chain_band_counts(msgpu_ctx *ctx, uint64_t *n_banded, uint64_t *n_fallback);
int msgpu_chain_band_width(void); /* B, a build-time constant (MSGPU_CHAIN_BAND) */
/* The candidate stage hands the chain stage one word per EdgeMatch (both row ranks, sixteen bits each) unless the job has a
 * read of more than 65,535 rows: 1 = the host keeps the ranks in two arrays for a job whose largest read has that many rows.
 * MSGPU_CAND_WIDE=1 forces that form. */
int msgpu_cand_wide(uint32_t largest_read_cnt);
/* The chain kernels leave an order as the four overhangs of its path (L1, L2 of the first anchor on v1 / v2, R1, R2 of the last,
 * the v2 side chosen by direction), its score as a double and raw_flags = MSGPU_ORD_DIR | MSGPU_ORD_PRIMARY; the compaction
 * kernel makes the msgpu_order of them.  This is that arithmetic on the host (the same function, compiled for both): fills
 * flags, left_offset, right_offset, score, start, end and base of *out and leaves its other fields alone; returns 1 when
 * getOverlap has a case for the four values (always, unless one is a NaN), else 0.  score must lie in [0, 2^64). */
int msgpu_order_finish(uint32_t raw_flags, double score, double L1, double L2, double R1, double R2, uint32_t v1, uint32_t v2,
                       msgpu_order *out);
/* The stage boundaries (index / candidates / chain / compact) are marked with HIP events on the context's stream; every
 * marker costs a few microseconds of command-processor time.  on = 0 drops them: msgpu_get_timings then reports only
 * chain_kernel_ms (the two events around the chain kernels stay) and zeros for the stages.  Default: on. */
int msgpu_set_stage_events(msgpu_ctx *ctx, int on);

/* Copy result tables to HOST buffers sized from msgpu_get_counts (any pointer may be NULL to skip). */
int msgpu_copy_tables(msgpu_ctx *ctx, msgpu_edge *edges, msgpu_edgematch *ems, msgpu_order *orders, uint32_t *ids);
/* Same into DEVICE buffers (device-to-device on the context's stream; used in front of the RCCL all-gather).
 * Asynchronous: STREAM CONTRACT rule 3 applies to the destination buffers. */
int msgpu_copy_tables_device(msgpu_ctx *ctx, void *d_edges, void *d_ems, void *d_orders, void *d_ids);
/* Per-read Vertex facts: Vertex::getNanoporeLength() and metaDatum(0) (first line), n_reads entries each (host). */
int msgpu_copy_reads(msgpu_ctx *ctx, int32_t *read_len, uint32_t *read_first_line);

/* Multi-GPU merge of the edge list (north_star: "a single RCCL all-gather over xGMI to merge the edge list").
 * Input: the result of ONE all-gather of equally sized slabs, slab r (from rank r) at d_gathered + r*slab_bytes,
 * holding that rank's edge / order / id tables at off_edges / off_orders / off_ids (padding after each is ignored).
 * counts = world x {n_edges, n_orders, n_ids} (host).  Output (device): dense rank-major tables with order_off,
 * edge_idx and ids_off re-based to the merged tables; em_off stays rank-local (EdgeMatch tables are not gathered).
 * The reference has no counterpart (single process); consumed like graph.getEdges() + Edge::getEdgeOrders().
 * Asynchronous: STREAM CONTRACT rule 3 applies to d_gathered (read) and to d_edges / d_orders / d_ids (written). */
int msgpu_merge_gathered(msgpu_ctx *ctx, const void *d_gathered, uint32_t world, const uint64_t *counts,
                         uint64_t slab_bytes, uint64_t off_edges, uint64_t off_orders, uint64_t off_ids, void *d_edges,
                         void *d_orders, void *d_ids);

/* The same with (a) id bases: id_base = world x {read id base, anchor id base} (NULL = zeros) is added to the read ids
 * (v1, v2, start, end, base) and to the anchor ids of rank r's records -- the ranks hold PARTITIONS of a larger job
 * (disjoint sets of reads and anchors, e.g. chromosomes: no edge crosses a partition), each with ids from 0, and the merged
 * list is the larger job's, (v1, v2)-sorted when the bases ascend; (b) the stream the merge kernel runs on (NULL = the
 * context's), so that an exchange can run on its own stream beside the next batch's compute. */
int msgpu_merge_gathered_ex(msgpu_ctx *ctx, const void *d_gathered, uint32_t world, const uint64_t *counts,
                            uint64_t slab_bytes, uint64_t off_edges, uint64_t off_orders, uint64_t off_ids,
                            const uint32_t *id_base, void *d_edges, void *d_orders, void *d_ids, void *hip_stream);

/* The exchange's WIRE FORM: the same merge with about 30 % fewer bytes over xGMI.  What a receiver can derive is not sent:
 * a rank's tables are dense (every record's slice of the next table starts where the one before ends), so the 64-bit
 * offsets travel as 32-bit CSR columns of n + 1 entries and the counts are their differences; an EdgeOrder's start / end /
 * base vertices follow from its flags and its edge (src/main.cpp:397-411: base = the edge's first vertex); padding is not
 * sent.  Columns, in this order, every block densely packed for the rank's OWN record count n:
 *   edge block  (msgpu_wire_edges_bytes(n)  = 17 n + 8): em_off[n+1] u32 | order_off[n+1] u32 | v1[n] | v2[n] | shadow[n] u8
 *   order block (msgpu_wire_orders_bytes(n) = 33 n + 4): left[n] f64 | right[n] f64 | score[n] u64 | ids_off[n+1] u32 |
 *                                                        edge_idx[n] u32 | flags[n] u8
 *   id block    (msgpu_wire_ids_bytes(n, id_bytes)): id_bytes = 4: as in the tables (4 n); id_bytes = 3, while the job's
 *               anchor ids fit 24 bits: four ids in three words (3 n, rounded up to a word) -- the ids are half of the
 *               wire slab, so this takes another 13 % off it.  Every rank of an exchange must use the same id_bytes.
 * msgpu_pack_wire writes the context's tables (after msgpu_chaining_and_overlaps) in that form into three DEVICE blocks
 * (edge and id blocks 4-byte, order block 8-byte aligned) on the context's stream; MSGPU_E_ARG when a table has more than
 * 2^32 - 1 EdgeMatches, orders or ids (exchange such tables whole) or, with id_bytes = 3, an anchor id space beyond 2^24.  msgpu_merge_wire = msgpu_merge_gathered_ex over
 * slabs whose three blocks are in wire form: the merged tables are the same, byte for byte (d_edges and d_orders 16-byte
 * aligned: the records leave as whole lines).
 * Both are asynchronous: STREAM CONTRACT rule 3 applies to the three blocks msgpu_pack_wire writes (a fill of those
 * buffers queued on another stream races with the pack kernel) and to msgpu_merge_wire's input and output buffers.
 * A table without records still sends its closing CSR entries (zeros): 8 bytes of the edge block, 4 of the order block. */
uint64_t msgpu_wire_edges_bytes(uint64_t n_edges);
uint64_t msgpu_wire_orders_bytes(uint64_t n_orders);
uint64_t msgpu_wire_ids_bytes(uint64_t n_ids, uint32_t id_bytes);
int msgpu_pack_wire(msgpu_ctx *ctx, void *d_wire_edges, void *d_wire_orders, void *d_ids, uint32_t id_bytes);
int msgpu_merge_wire(msgpu_ctx *ctx, const void *d_gathered, uint32_t world, const uint64_t *counts, uint64_t slab_bytes,
                     uint64_t off_edges, uint64_t off_orders, uint64_t off_ids, uint32_t id_bytes, const uint32_t *id_base,
                     void *d_edges, void *d_orders, void *d_ids, void *hip_stream);
/* The receiving end on the HOST: one set of wire blocks (host memory) back into records, on up to `threads` host threads (0 = 16).
 * base[4] = what precedes the set in the tables its records point into {edges, EdgeMatches, orders, ids}: added to edge_idx,
 * em_off, order_off, ids_off (NULL = zeros: the records of msgpu_copy_tables for the same context).  tables: which of them to
 * write -- 1 edges, 2 orders, 4 ids, 0 = all; a caller whose blocks arrive one after the other unpacks each as it lands (the
 * orders read the edge BLOCK for their vertices, not the edge records).  msgpu_overlap_batched_ex uses it for its windows
 * when the EdgeMatch table stays in HBM, msgpu_group_overlap for every member's slab (the tables travel over the host link in
 * wire form).  No GPU, no context: plain host code. */
int msgpu_unpack_wire_host(const void *wire_edges, const void *wire_orders, const void *wire_ids, uint32_t id_bytes,
                           uint64_t n_edges, uint64_t n_orders, uint64_t n_ids, const uint64_t *base, msgpu_edge *edges,
                           msgpu_order *orders, uint32_t *ids, uint32_t threads, uint32_t tables);

/* ---- one process, the node's GPUs: a GROUP of contexts behind the same call site -------------------------------------------
 * The reference is ONE process that fans jobs over its workers and closes each phase with a barrier (src/main.cpp:143-178,
 * libms/src/threading/ThreadPool.cpp:38-129, WaitGroup.cpp:62-72).  Its multi-GPU equivalent: one process, one context per
 * device, one host thread per device for the duration of a call, and ONE collective on the results (with several members a
 * second, input-side one completes the row table in every HBM).  msgpu_group_overlap =
 *   rows (host) -> a 1/n-th over each device's own link, completed in every HBM by a grouped in-place all-gather over xGMI
 *   (MSGPU_GROUP_ROWS=replicate at creation, a group of one, or fewer than 1024 rows: the whole table over every link) ->
 *   index build on every device (replicated: a member needs
 *   the rank of every row inside its read) -> device i computes the edges with v1 % n == i (msgpu_set_shard) -> its edge /
 *   order / id tables in WIRE FORM into its slab (msgpu_pack_wire) -> ONE grouped RCCL all-gather over xGMI
 *   (ncclGroupStart / n x ncclAllGather / ncclGroupEnd, each on its member's stream) -> msgpu_merge_wire on every device:
 *   the merged edge list of the job in every HBM, and in host memory (every member sends its OWN slab, still in wire form,
 *   over its own link beside the exchange; host threads turn the slabs into the merged records: msgpu_unpack_wire_host with
 *   the member's bases); WaitGroup::wait() = the join of the member threads.
 * The merged tables are the ones msgpu_merge_wire defines: rank-major (member 0's edges in (v1, v2) order, then member 1's ...),
 * order_off / edge_idx / ids_off re-based to the merged tables, em_off local to the owning member (EdgeMatch tables are not
 * gathered: msgpu_get_edgematches on msgpu_group_ctx(g, v1 % n)).  With n = 1 they are the single-context tables bit for bit.
 * RCCL is loaded on first use (dlopen of librccl.so.1: the process's own copy where a framework already brought one); a
 * process that never creates a group never maps it.  MSGPU_E_NODEVICE when a device is missing, MSGPU_E_HIP with the RCCL
 * error text when a collective fails.  A group is driven by one host thread at a time (STREAM AND THREAD CONTRACT rule 5);
 * the members' contexts must not be used by the caller while a group call runs.
 * Rehearsal on a box with fewer GPUs than members: with MSGPU_GROUP_TRANSPORT=copy in the environment when the group is
 * created, the all-gather is carried by device-to-device copies of this process instead of RCCL and members may share a device;
 * shards, threads, slab layout, pack and merge are the same code.  For tests; never the default. */
typedef struct msgpu_group msgpu_group;
typedef struct msgpu_group_tables {
  const msgpu_edge  *edges;   /* host (pinned, owned by the group, valid until its next call): the merged edge list     */
  const msgpu_order *orders;
  const uint32_t    *ids;
  const int32_t     *read_len;        /* Vertex::getNanoporeLength(), n_reads entries                                  */
  const uint32_t    *read_first_line; /* Vertex::metaDatum(0)                                                          */
  uint64_t n_edges, n_orders, n_ids, n_ems; /* n_ems: EdgeMatches over all members (the tables stay in their HBMs)     */
  uint32_t n_reads, n_anchors, n_members, id_bytes; /* id_bytes: 3 or 4, how anchor ids travelled                      */
  uint64_t slab_bytes;        /* bytes every member sent (the largest member's wire blocks)                            */
  float wall_ms;              /* host clock: call entry -> merged tables in host memory                                */
  float compute_ms;           /*   slowest member: rows in HBM + index + its shard                                     */
  float exchange_ms;          /*   slowest member: pack + all-gather + merge (device time, HIP events)                 */
  uint32_t rows_sliced;       /* 1: every member took a 1/n-th of the rows over its link, an all-gather did the rest   */
} msgpu_group_tables;
int  msgpu_group_create(const int *devices, int n, const msgpu_params *params, msgpu_group **out);
void msgpu_group_destroy(msgpu_group *g);
const char *msgpu_group_last_error(const msgpu_group *g);
int  msgpu_group_size(const msgpu_group *g);
msgpu_ctx *msgpu_group_ctx(msgpu_group *g, int member); /* member i's context: its counts, its EdgeMatch table, its merged device tables */
int  msgpu_group_overlap(msgpu_group *g, const msgpu_row *rows, size_t n_rows, msgpu_group_tables *out);
/* A way out of a collective that never completes.  timeout_ms > 0: msgpu_group_overlap gives up that long after its entry --
 * every host wait of the call (the members' table sizes, the slabs landing in host memory, the closing barrier) polls instead of
 * blocking -- then aborts the members' communicators (ncclCommAbort: the collective's kernels leave the streams), waits at most
 * the same time again for the streams to drain, and returns MSGPU_E_TIMEOUT with the text saying whether they did.  The next call
 * builds fresh communicators.  0 = wait for ever (the default; MSGPU_GROUP_TIMEOUT_MS in the environment at creation sets
 * another).  The one-catch error model of src/main.cpp:313-315: the caller sees a code, not a process that hangs.
 * On ANY error return the group has synchronised what it queued where that was possible (nothing of the call reads `rows` or
 * writes the group's host tables any more unless the text says the streams did not drain); the calling thread's current HIP
 * device is restored on every return. */
int  msgpu_group_set_timeout(msgpu_group *g, uint32_t timeout_ms);
/* The merged tables as member `member` holds them in ITS HBM (device pointers, valid until the group's next call): what
 * msgpu_find_contraction_edges(msgpu_group_ctx(g, member), d_edges, n_edges, d_orders, n_orders, n_reads, ...) takes. */
int  msgpu_group_device_tables(msgpu_group *g, int member, const void **d_edges, const void **d_orders, const void **d_ids);

/* ---- the ThreadPool replacement: the whole overlap path, host memory to host memory, as batches on two HIP streams ----
 * Replaces the phases of src/main.cpp:153-178 that the reference fans over its ThreadPool (one Job per PAF line, per
 * anchor, per edge; libms/src/threading/ThreadPool.cpp:38-129) and closes with WaitGroup::wait() (WaitGroup.cpp:62-72):
 *   rows -> HBM and index build once (msgpu_load_rows), then n_batches windows of owner reads, each one
 *   msgpu_calculate_edges + msgpu_chaining_and_overlaps on the compute stream, while the previous window's edge /
 *   EdgeMatch / order / id tables are copied to pinned host memory on a second stream (two table sets in HBM).
 * The call returns when every batch is done (the phase barrier).  The host tables are the single-pass tables of
 * msgpu_copy_tables bit for bit -- canonical order, cross references (em_off, order_off, edge_idx, ids_off) into the
 * whole tables -- owned by the context and valid until its next msgpu_overlap_batched / msgpu_destroy.  HBM holds one
 * window's tables at a time instead of the job's.  With msgpu_set_shard the windows cut this shard's reads.
 * The windows are cut by measured work (the index build counts, per read, the scaffold rows it visits as an owner), so they
 * hold the shares wanted whatever the read ids have to do with genome position.
 * n_batches 0 = 8 (3 with MSGPU_BATCH_NO_EDGEMATCHES).  `rows` should be pinned (msgpu_pinned_alloc) for the copy to run at link speed. */
typedef struct msgpu_host_tables {
  const msgpu_edge      *edges;
  const msgpu_edgematch *ems;
  const msgpu_order     *orders;
  const uint32_t        *ids;
  const int32_t         *read_len;        /* Vertex::getNanoporeLength(), n_reads entries */
  const uint32_t        *read_first_line; /* Vertex::metaDatum(0) */
  uint64_t n_edges, n_ems, n_orders, n_ids;
  uint32_t n_reads, n_anchors, n_batches, pad;
  float wall_ms;         /* host clock: call entry -> all tables in host memory */
  float load_ms;         /*   of which rows -> HBM + index build */
  float first_batch_ms;  /*   first window computed (its copy starts here) */
  float compute_done_ms; /*   last window computed (what remains is copy) */
} msgpu_host_tables;
int msgpu_overlap_batched(msgpu_ctx *ctx, const msgpu_row *rows, size_t n_rows, uint32_t n_batches,
                          msgpu_host_tables *out);
/* The same with options (flags = 0: msgpu_overlap_batched).
 *   MSGPU_BATCH_RESIDENT        the job's four tables stay WHOLE in HBM (window k writes behind window k-1; 288 GB of HBM
 *                               hold the 1 GB of BASELINE.json configs[2] many times over): no second table set, the
 *                               compute stream never waits for a copy, and afterwards the context is in the state
 *                               msgpu_chaining_and_overlaps leaves -- msgpu_find_contraction_edges, msgpu_copy_tables
 *                               [_device], msgpu_get_edgematches and msgpu_get_counts work on the job's tables.
 *   MSGPU_BATCH_NO_EDGEMATCHES  (implies RESIDENT) the EdgeMatch table is NOT copied to the host: out->ems = NULL,
 *                               out->n_ems is still its size.  Downstream only assemblePath reads EdgeMatches, and only
 *                               those of path edges (dg.cpp:99-101 -> ap.cpp:631-706): fetch them with
 *                               msgpu_get_edgematches.  The other three tables cross the host link in the exchange's
 *                               wire form (msgpu_pack_wire per window; 93 MB instead of 154 MB -- or 971 MB with the
 *                               EdgeMatches -- on configs[2]) and a host thread of the call turns every window back
 *                               into records (msgpu_unpack_wire_host) while the next one computes: the tables handed
 *                               out are the same records.  MSGPU_NO_WIRE_COPY=1 in the environment of msgpu_create:
 *                               whole records over the link (A/B switch).
 *   MSGPU_BATCH_ROWS_ON_DEVICE  `rows` is a DEVICE pointer (msgpu_load_rows_device): the table is in HBM already, e.g.
 *                               all-gathered over xGMI from the 1/N slices the ranks of a node uploaded over their own links.
 *   MSGPU_BATCH_ROWS_PACKED     `rows` points to a msgpu_packed_rows (below) and n_rows is its n_rows: 28 bytes per row over
 *                               the host link instead of 40 (msgpu_load_rows_packed).
 */
#define MSGPU_BATCH_RESIDENT 1u
#define MSGPU_BATCH_NO_EDGEMATCHES 2u
#define MSGPU_BATCH_ROWS_ON_DEVICE 4u
#define MSGPU_BATCH_ROWS_PACKED 8u
int msgpu_overlap_batched_ex(msgpu_ctx *ctx, const msgpu_row *rows, size_t n_rows, uint32_t n_batches, uint32_t flags,
                             msgpu_host_tables *out);
/* MatchMap::getEdgeMatches(edge) (libms/src/matching/MatchMap.cpp:136-159) for a LIST of edges, from the EdgeMatch table
 * resident in HBM (after msgpu_chaining_and_overlaps or a resident msgpu_overlap_batched_ex): one gather kernel + one
 * copy.  edge_idx[i] = index in the edge table.  *em_off (n + 1 entries) / *ems: the EdgeMatches of edge_idx[i] are
 * (*ems)[(*em_off)[i] .. (*em_off)[i+1]), in table order (edge_idx of each record is unchanged).  Both arrays are pinned
 * host memory owned by the context, valid until its next msgpu_get_edgematches / msgpu_destroy. */
int msgpu_get_edgematches(msgpu_ctx *ctx, const uint32_t *edge_idx, size_t n, const uint64_t **em_off,
                          const msgpu_edgematch **ems);
/* page-locked host memory for rows handed to msgpu_load_rows / msgpu_overlap_batched (NULL when out of memory) */
void *msgpu_pinned_alloc(size_t bytes);
void  msgpu_pinned_free(void *p);

/* findContractionEdges (src/main.cpp:183-190, 416-463) with sanityCheck (libms/src/kernel/sc.cpp:29-90) -- the step
 * that follows the chaining fan-out -- on an edge/order table resident in HBM.  contraction_order (host, n_edges
 * entries): for every edge the index in the order table of its first contained & primary EdgeOrder that is sane against
 * every non-shadow neighbour of the order's start vertex (what the reference inserts into `contractionEdges`), or -1.
 * d_edges = d_orders = NULL: the context's own tables (single GPU, after msgpu_chaining_and_overlaps); otherwise any
 * (v1, v2)-sorted edge table + its order table, e.g. the merged list of msgpu_merge_gathered; n_reads = max id + 1.
 * Uses msgpu_params.wiggle_room.  Synchronous for the host; caller tables are read in the context's stream order
 * (STREAM CONTRACT rule 3 (a): they must be complete there). */
int msgpu_find_contraction_edges(msgpu_ctx *ctx, const void *d_edges, uint64_t n_edges, const void *d_orders,
                                 uint64_t n_orders, uint32_t n_reads, int64_t *contraction_order);

/* Block the host until everything queued on the context's stream has finished. */
int msgpu_synchronize(msgpu_ctx *ctx);
/* A deadline for the host waits of this context: from now on, and until the next msgpu_set_deadline, every wait a call of this
 * context makes for its stream (table sizes coming back in msgpu_load_rows* / msgpu_calculate_edges /
 * msgpu_chaining_and_overlaps, msgpu_synchronize, msgpu_copy_reads) gives up `timeout_ms` after THIS call and returns
 * MSGPU_E_TIMEOUT; 0 = no deadline (the default: the runtime's blocking waits).  Nothing is cancelled: the work stays queued,
 * the caller removes what holds the stream up (e.g. aborts its collective) and synchronises, or destroys the context.  Exists
 * for contexts whose stream also carries somebody else's collective (msgpu_group_overlap sets it from the group's timeout). */
int msgpu_set_deadline(msgpu_ctx *ctx, uint32_t timeout_ms);
/* A gate for a caller's OTHER thread that has device work of its own to place (an exchange of the previous job's tables, say):
 * msgpu_chain_launches = how often msgpu_chaining_and_overlaps has launched its chain kernels so far; msgpu_wait_chain_launch
 * blocks the calling thread until that count reaches `count` (0) or `timeout_us` has passed (1).  The chain stage is bound by
 * instruction issue, the stages before it by memory: work enqueued on another stream when the wait returns runs beside the
 * stage that has bandwidth to spare (bench.py --gpus N: the merge of step k's gathered slabs beside the chain stage of step
 * k + 1; the all-gather itself, bound by the links, is not held).  The two calls may be made from any thread while another thread drives the context (the one exception to rule 5 of
 * the STREAM AND THREAD CONTRACT besides msgpu_merge_*_ex); they touch nothing but the counter. */
uint64_t msgpu_chain_launches(msgpu_ctx *ctx);
int msgpu_wait_chain_launch(msgpu_ctx *ctx, uint64_t count, uint32_t timeout_us);

/* ---- for tests: the context's device buffers --------------------------------------------------------------------
 * One text line per device buffer of the context, in the order of the buffer table in csrc/msgpu_api.hip:
 *   "<name> <bytes> <guarded 0|1> <carries 0|1> <generation>\n"
 * bytes: the size of the block the buffer holds now (0: none); guarded: the block lies between guards (it was allocated
 * under MSGPU_POISON: exactly as large as the request, filled with 0xA5, and every entry that launches work compares its
 * guards before it returns MSGPU_OK -- a written one is MSGPU_E_HIP with a text that begins with "arena guard:"); carries:
 * the buffer carries something across the start of a job (the table says what) and is not given back there; generation: the
 * allocations made through this buffer so far.  The text is cut to text_bytes - 1 characters and closed with a 0;
 * *needed (may be NULL) = the bytes the whole text takes, the 0 included.  No device work. */
int msgpu_debug_buffers(msgpu_ctx *ctx, char *text, size_t text_bytes, size_t *needed);

/* ==== sequence store + slice / reverse-complement / stitch kernel: device half of the "consensus" stage (A9) ========
 *
 * assemblePath (libms/src/kernel/ap.cpp:615-1362) decides where every piece of sequence goes; the bytes come from
 *   SequenceAccessor::buildIndex / get{Nanopore,Illumina}Sequence(id)     SequenceAccessor.cpp:54-69,114-231
 *   strSlice, getReverseComplement, get{Illumina,Nanopore}Sequence(l,r,d)  SequenceUtils.cpp:27-85
 *   updateConsensusBase (prepend / append the uncovered part)              ap.cpp:205-229
 * Here: the files are parsed once on the host (msgpu_seq_parse), every record lives whitespace-free in HBM
 * (msgpu_seq_upload), and a whole batch of pieces is produced by ONE kernel launch (msgpu_gather_run). */

typedef struct msgpu_seqfile msgpu_seqfile;     /* a parsed FASTA/FASTQ file on the host              */
typedef struct msgpu_seqctx msgpu_seqctx;       /* the two sequence stores (nanopore, illumina) in HBM */
typedef struct msgpu_gather_plan msgpu_gather_plan;

/* Replaces SequenceAccessor::_buildNanoporeIdx/_buildIlluminaIdx + getSequenceFromFile.  is_fastq: 1, 0, or -1 to
 * decide from the extension like isFastQ (SequenceAccessor.cpp:71-80: FASTQ unless ".fa"/".fasta"). */
int         msgpu_seq_parse(const char *path, int is_fastq, msgpu_seqfile **out);
void        msgpu_seq_free(msgpu_seqfile *f);
uint32_t    msgpu_seq_count(const msgpu_seqfile *f);
const char *msgpu_seq_name(const msgpu_seqfile *f, uint32_t record);   /* cleaned id (cut at the first whitespace) */
uint64_t    msgpu_seq_length(const msgpu_seqfile *f, uint32_t record);
const char *msgpu_seq_bases(const msgpu_seqfile *f, uint32_t record);  /* not NUL-terminated                       */
/* the one buffer every record's bytes lie in (msgpu_seq_bases points into it; records need not touch each other) and
 * its used size: what msgpu_seq_upload copies to HBM */
const char *msgpu_seq_buffer(const msgpu_seqfile *f, uint64_t *bytes);
uint64_t    msgpu_seq_offset(const msgpu_seqfile *f, uint32_t record);  /* of the record's bytes inside that buffer */

/* strSlice (SequenceUtils.cpp:27-38) as (returned offset, *len): Python-like indices, INCLUSIVE clipped end. */
uint64_t msgpu_str_slice(uint64_t size, int32_t start, int32_t end, uint64_t *len);

/* device = HIP ordinal (MSGPU_E_NODEVICE without a GPU), or -1 for a layout-only context: the slice arithmetic and the
 * segment composers below work on it, but nothing can be uploaded to or gathered on a device. */
int         msgpu_seq_create(int device, msgpu_seqctx **out);
void        msgpu_seq_destroy(msgpu_seqctx *ctx);
const char *msgpu_seq_last_error(const msgpu_seqctx *ctx);
/* kind 0 = nanopore reads, 1 = illumina unitigs.  ids[record] = Registry id of that record (0xffffffff = skip);
 * NULL = record order.  n_ids = size of the id space. */
int msgpu_seq_upload(msgpu_seqctx *ctx, int kind, const msgpu_seqfile *f, const uint32_t *ids, uint32_t n_ids);
/* The same in two steps, for a caller that parses the sequence files beside the PAF (SequenceAccessor::buildIndex needs
 * the Registry only for the ids, SequenceAccessor.cpp:171,215): the bytes as soon as a file is parsed -- the two kinds may
 * be sent (and converted, msgpu_seq_pack_store) from two host threads at the same time --, the ids of the SAME file once
 * the registries exist (MSGPU_E_STATE when the store holds another file's bytes). */
int msgpu_seq_upload_bases(msgpu_seqctx *ctx, int kind, const msgpu_seqfile *f);
/* msgpu_seq_parse + msgpu_seq_upload_bases in one pass over the file: the parser's threads strip the records into a ring
 * of page-locked slots that travel to the store while the file is still being read; the host never holds the bases.  The
 * msgpu_seqfile that comes back has names, lengths and offsets (msgpu_seq_set_ids and msgpu_paf_register_sequences take
 * it) but no bytes: msgpu_seq_bases and msgpu_seq_buffer return NULL for it. */
int msgpu_seq_parse_upload(msgpu_seqctx *ctx, int kind, const char *path, int is_fastq, msgpu_seqfile **out);
int msgpu_seq_set_ids(msgpu_seqctx *ctx, int kind, const msgpu_seqfile *f, const uint32_t *ids, uint32_t n_ids);

/* Same from a device buffer that already holds the whitespace-free bases (copied device-to-device into the store):
 * off[id] / len[id] = position of sequence `id` inside it (off = ~0 for an id without sequence). */
int msgpu_seq_upload_device(msgpu_seqctx *ctx, int kind, const void *d_bases, uint64_t n_bases, const uint64_t *off,
                            const uint64_t *len, uint32_t n_ids);

/* Convert both resident stores to 2 bits per base (A C G T) plus a sorted list of the positions holding any other byte
 * (N, lower case, IUPAC: reproduced verbatim), and free the byte-per-base copies: a quarter of the HBM footprint and
 * 1.25 instead of 2 bytes of traffic per gathered base.  Results of every later gather are unchanged.  A new upload
 * returns the store to the byte form. */
int msgpu_seq_pack(msgpu_seqctx *ctx);
int msgpu_seq_pack_store(msgpu_seqctx *ctx, int kind); /* one store only */

/* One piece of output: `len` bases starting at `src_off` of a store, as they are or reverse-complemented, written
 * at dst_off.  24 bytes. */
typedef struct msgpu_copy {
  uint64_t src_off; /* first source base, offset inside the store                     */
  uint64_t dst_off; /* first output byte                                               */
  uint32_t len;
  uint32_t flags;   /* MSGPU_COPY_*                                                    */
} msgpu_copy;
#define MSGPU_COPY_ILLUMINA 1u /* source store: illumina (else nanopore)                */
#define MSGPU_COPY_REVCOMP 2u  /* reverse complement (direction == false)               */

/* get{Nanopore,Illumina}Sequence(seq_id, left, right, direction) (SequenceUtils.cpp:63-85) as a piece: fills src_off,
 * len and flags of *out (dst_off is the caller's layout decision). */
int msgpu_seq_resolve(msgpu_seqctx *ctx, int kind, uint32_t seq_id, int32_t left, int32_t right, int direction,
                      msgpu_copy *out);

/* The segment builders of assemblePath as piece composers (libms/src/kernel/ap.cpp:191-203, 352-579).  m / ml / mr =
 * the read's VertexMatch rows on the anchor(s) (read_id, anchor_id, ranges, direction bit); ov* = the anchor's
 * overlap from Id2OverlapMap; direction = the read's orientation in the layout (Vertex::getVertexDirection() == e_POS).
 * `out` receives the pieces in output order with dst_off relative to the start of the segment (up to 1 / 2 / 2 / 3
 * pieces); add the segment's position in the output to every dst_off before planning the gather. */
int msgpu_seg_anchor(msgpu_seqctx *ctx, const msgpu_row *m, int32_t ov_lo, int32_t ov_hi, int direction,
                     msgpu_copy *out, uint32_t *n_out, uint64_t *len);                       /* getAnchorSequence        */
int msgpu_seg_left_of_anchor(msgpu_seqctx *ctx, const msgpu_row *m, uint64_t nanopore_length, int32_t ov_lo,
                             int32_t ov_hi, int direction, msgpu_copy *out, uint32_t *n_out,
                             uint64_t *len);                                                  /* getSequenceLeftOfAnchor  */
int msgpu_seg_right_of_anchor(msgpu_seqctx *ctx, const msgpu_row *m, uint64_t nanopore_length, int32_t ov_lo,
                              int32_t ov_hi, int direction, msgpu_copy *out, uint32_t *n_out,
                              uint64_t *len);                                                 /* getSequenceRightOfAnchor */
/* getSequenceBetweenAnchors: *has_sequence = 0 mirrors std::nullopt; *distance = std::get<0> of its result. */
int msgpu_seg_between_anchors(msgpu_seqctx *ctx, const msgpu_row *ml, const msgpu_row *mr, int32_t ovl_lo,
                              int32_t ovl_hi, int32_t ovr_lo, int32_t ovr_hi, int direction, msgpu_copy *out,
                              uint32_t *n_out, int32_t *distance, int *has_sequence);

/* updateConsensusBase (ap.cpp:205-229) on piece lists: the growing contig of visitOrdered as (pieces, borderLeft,
 * borderRight).  An update takes the new sequence as a segment (pieces with segment-relative dst_off, e.g. what the
 * msgpu_seg_* composers return) plus its borders and prepends / appends the part the contig does not cover yet. */
typedef struct msgpu_consensus msgpu_consensus;
msgpu_consensus *msgpu_consensus_new(void);
void             msgpu_consensus_free(msgpu_consensus *c);
int msgpu_consensus_update(msgpu_consensus *c, const msgpu_copy *seg, uint32_t n, int32_t new_lo, int32_t new_hi);
int msgpu_consensus_borders(const msgpu_consensus *c, int32_t *lo, int32_t *hi, uint64_t *length);
/* The contig as pieces laid out from dst_off = base; returns the piece count (call with out = NULL to size). */
size_t msgpu_consensus_pieces(const msgpu_consensus *c, uint64_t base, msgpu_copy *out, size_t cap);
msgpu_consensus *msgpu_consensus_clone(const msgpu_consensus *c);

/* Upload a batch of pieces (+ its work partition) once; run it any number of times. */
int      msgpu_gather_plan_create(msgpu_seqctx *ctx, const msgpu_copy *pieces, size_t n, msgpu_gather_plan **out);
void     msgpu_gather_plan_free(msgpu_gather_plan *plan);
uint64_t msgpu_gather_plan_out_bytes(const msgpu_gather_plan *plan); /* max(dst_off + len)  */
uint64_t msgpu_gather_plan_bases(const msgpu_gather_plan *plan);     /* sum(len)            */
/* d_out: device buffer of out_capacity >= out_bytes.  hip_stream NULL = the context's stream. Asynchronous. */
int msgpu_gather_run(msgpu_seqctx *ctx, const msgpu_gather_plan *plan, void *d_out, uint64_t out_capacity,
                     void *hip_stream);
int msgpu_seq_synchronize(msgpu_seqctx *ctx);

/* ---- assemblePath (libms/src/kernel/ap.cpp:615-1362; caller assemblePathsSub, src/main.cpp:663-677) ---------------
 * One msgpu_assembly collects any number of paths.  msgpu_assembly_add_path runs the reference's layout decisions on
 * the host for one path (candidate EdgeOrders, anchor cliques, the anchor DAG, placement, flanks, contained reads) and
 * records every output sequence as copy pieces; it reads no base.  msgpu_assembly_finish then produces all bases of
 * all paths with ONE gather launch and wraps them into FASTA text on the device (60 columns, ap.cpp:52,61-76):
 * the texts are what OutputWriter::writeTarget / writeQuery / writePaf (OutputWriter.cpp:49-62) receive, in path order.
 *
 * Hash-order note: where ap.cpp iterates std::unordered_map / unordered_set (graph vertices, edges, successors, tap
 * entries) the reference's order is unspecified; this library uses ascending ids / creation order ("canonical order"). */
typedef struct msgpu_path_read {
  uint32_t read_id;          /* Vertex::getId()                                         */
  uint32_t direction;        /* Vertex::getVertexDirection(): 1 = e_POS, 0 = e_NEG, 2 = e_NONE */
  uint64_t nanopore_length;  /* Vertex::getNanoporeLength()                             */
} msgpu_path_read;
typedef struct msgpu_path_order { /* an EdgeOrder (include/ms/graph/Edge.h:49-60) of a directed path edge */
  uint64_t score;
  uint32_t base_read; /* baseVertex id                                                 */
  uint32_t ids_off;   /* its ids = ids[ids_off .. ids_off + ids_cnt)                   */
  uint32_t ids_cnt;
  uint32_t pad;
} msgpu_path_order;
typedef struct msgpu_path_em { /* EdgeMatch::overlap of a path edge on one anchor, MatchMap.h:68-74 */
  uint32_t anchor_id;
  int32_t  ov_lo, ov_hi;
} msgpu_path_em;
typedef struct msgpu_path_contain { /* a ContainElement (MatchMap.h:80-87) attached to a read of the path */
  uint32_t host_read;   /* the path read that contains it                              */
  uint32_t nano;        /* the contained read                                          */
  uint32_t direction;   /* ContainElement::direction                                   */
  uint32_t anchors_off; /* keys of ContainElement::matches = contain_anchors[off .. off + cnt); the VertexMatch of */
  uint32_t anchors_cnt; /* (nano, anchor) is looked up in `rows`                       */
} msgpu_path_contain;
typedef struct msgpu_path_input {
  const msgpu_path_read  *reads;     /* the path, n_reads >= 2                                              */
  uint32_t                n_reads;
  int32_t                 asm_idx;   /* asmIdx: names ">muchsalsa_<asmIdx>", ">Middle.<asmIdx>.<n>" ...     */
  const uint32_t         *order_off; /* n_reads entries: path edge i = reads[i] -> reads[i+1] owns orders   */
  const msgpu_path_order *orders;    /*   [order_off[i], order_off[i+1]) (diGraph.getEdge(..)->getEdgeOrders()) */
  const uint32_t         *ids;       /* id pool of the orders                                               */
  const uint32_t         *em_off;    /* n_reads entries: EdgeMatches of path edge i                         */
  const msgpu_path_em    *ems;
  const msgpu_row        *rows;      /* MatchMap::getVertexMatch source: the (read, anchor) rows of the path's reads */
  size_t                  n_rows;    /*   and of the contained reads (any order); optional after msgpu_assembly_set_rows */
  const msgpu_path_contain *contains;
  uint32_t                n_contains;
  uint32_t                pad;
  const uint32_t         *contain_anchors;
} msgpu_path_input;

typedef struct msgpu_assembly msgpu_assembly;
typedef struct msgpu_path_info {
  uint64_t target_len;     /* bases of the contig                                        */
  uint64_t target_raw_off; /* where its bases start in the raw (unwrapped) buffer        */
  uint32_t query_begin, query_end; /* its query records                                  */
  uint32_t n_anchors, n_anchor_edges;
  int32_t  border_lo, border_hi;   /* globalPos1, globalPos2 (ap.cpp:880-881)            */
  int32_t  asm_idx;
  uint32_t pad;
} msgpu_path_info;
#define MSGPU_QUERY_MIDDLE 0u
#define MSGPU_QUERY_LEFT 1u
#define MSGPU_QUERY_RIGHT 2u
#define MSGPU_QUERY_CONTAIN_ILLUMINA 3u
#define MSGPU_QUERY_CONTAIN_NANO 4u
typedef struct msgpu_query_info {
  uint64_t len;
  uint64_t raw_off;
  int64_t  lb, rb; /* PAF columns 8 and 9 as the reference prints them                   */
  uint32_t kind;   /* MSGPU_QUERY_*                                                      */
  uint32_t path;
} msgpu_query_info;

/* The assembly uses `ctx` until msgpu_assembly_finish / _validate have returned; freeing it never touches `ctx`. */
int         msgpu_assembly_create(msgpu_seqctx *ctx, msgpu_assembly **out);
void        msgpu_assembly_free(msgpu_assembly *a);
const char *msgpu_assembly_last_error(const msgpu_assembly *a);
/* Install the VertexMatch table once (MatchMap::getVertexMatch for every later path; copied, n_rows < 2^32).  A path's
 * own msgpu_path_input.rows, when given, are looked up first. */
int msgpu_assembly_set_rows(msgpu_assembly *a, const msgpu_row *rows, size_t n_rows);
/* The same without the copy: `rows` (e.g. msgpu_paf_rows of a live msgpu_paf) stays the caller's and must outlive the
 * assembly's last msgpu_assembly_add_path(s).  The reference's MatchMap hands out pointers into its own table the same way. */
int msgpu_assembly_borrow_rows(msgpu_assembly *a, const msgpu_row *rows, size_t n_rows);
/* MSGPU_E_LAYOUT leaves the assembly unchanged (the path is skipped). */
int      msgpu_assembly_add_path(msgpu_assembly *a, const msgpu_path_input *in);
/* The assemblePaths fan-out (src/main.cpp:620-677): n paths laid out by n_threads host threads, appended in input
 * order.  status (optional, n entries) receives each path's result; MSGPU_E_LAYOUT paths are skipped.  Returns the
 * first status that is neither MSGPU_OK nor MSGPU_E_LAYOUT, else MSGPU_OK. */
int msgpu_assembly_add_paths(msgpu_assembly *a, const msgpu_path_input *in, size_t n, uint32_t n_threads, int *status);
uint32_t msgpu_assembly_path_count(const msgpu_assembly *a);
uint32_t msgpu_assembly_query_count(const msgpu_assembly *a);
int      msgpu_assembly_path_info(const msgpu_assembly *a, uint32_t path, msgpu_path_info *out);
int      msgpu_assembly_query_info(const msgpu_assembly *a, uint32_t query, msgpu_query_info *out);
/* every copy piece of every record, dst_off = position in the raw buffer; returns the count (out = NULL to size) */
size_t   msgpu_assembly_pieces(const msgpu_assembly *a, msgpu_copy *out, size_t cap);
uint64_t msgpu_assembly_raw_bytes(const msgpu_assembly *a);
/* gather + FASTA wrapping on the device, texts copied to host memory owned by the assembly.  hip_stream NULL = the
 * context's stream.  Synchronous.  MSGPU_E_NODEVICE on a layout-only context. */
int msgpu_assembly_finish(msgpu_assembly *a, void *hip_stream);
/* After finish: banded Levenshtein distance (msgpu_edit_distance semantics, band <= 127) of every query record against
 * the stretch of its contig that its PAF line names, clipped to the contig; distance[i] for query i (host, query_count
 * entries): the distance when <= band, else band + 1.  dp_cells (optional): DP cells inside the band that were evaluated.
 * No reference counterpart: it is the meter of how well the query records agree with the contig. */
int msgpu_assembly_validate(msgpu_assembly *a, uint32_t band, uint32_t *distance, uint64_t *dp_cells);
/* which: 0 = temp_1.target.fa, 1 = temp_1.query.fa (both after finish), 2 = temp_1.align.paf (after add_path) */
const char *msgpu_assembly_text(const msgpu_assembly *a, int which, uint64_t *len);

/* FASTA wrapping on the device: record r = header bytes, then `len` bases from d_raw + raw_off in lines of 60
 * (limitLength, ap.cpp:61-76), then '\n'; written at d_text + text_off.  Asynchronous on hip_stream / the ctx stream. */
typedef struct msgpu_fasta_record {
  uint64_t raw_off, text_off;
  uint32_t len;
  uint32_t header_off, header_len; /* header = headers[header_off .. +header_len), e.g. ">muchsalsa_1\n" */
  uint32_t pad;
} msgpu_fasta_record;
uint64_t msgpu_fasta_text_bytes(uint32_t header_len, uint64_t len);
int msgpu_fasta_format(msgpu_seqctx *ctx, const void *d_raw, const msgpu_fasta_record *records, size_t n,
                       const char *headers, size_t headers_bytes, void *d_text, uint64_t text_capacity,
                       void *hip_stream);

/* ==== unitig coverage filter: the pipeline's own step between the external tools and muchsalsa ==========================
 * Input: a unitig -> read PAF (every line counts; a block = a maximal run of consecutive lines with the same column 0) and
 * the unitig FASTA.  Pass 1 (device): per block, the maximum coverage over [0, qlen) by the FIRST line of each read id in
 * the block.  Per unitig id the value of its last block; q1 / q3 = numpy's linear percentile 25 / 75 over one value per
 * id, upper = q3 + 1.5 (q3 - q1).  Pass 2 (device): a block whose id's value exceeds upper is an outlier; its coverage by
 * ALL its lines is cut into maximal runs of cov <= q3, and runs of >= 500 positions become fragments.  Output (device
 * gather + FASTA wrapping): per block in PAF order, the unitig's whole record (normal) or its fragments (outlier). */
typedef struct msgpu_uf msgpu_uf;       /* a parsed filter PAF (host)                 */
typedef struct msgpu_ufctx msgpu_ufctx; /* a device context of the stage              */
typedef struct msgpu_uf_result msgpu_uf_result;
typedef struct msgpu_uf_tables { /* views into a msgpu_uf (valid while it lives)                                       */
  uint64_t        n_lines;
  uint32_t        n_blocks, n_unitigs, n_reads, pad;
  const uint32_t *line_block, *line_qs, *line_qe, *line_read;     /* per line; qe exclusive; ids first-seen          */
  const uint32_t *block_first, *block_n, *block_qlen, *block_unitig; /* per block; qlen = its first line's column 1 */
  const uint32_t *unitig_last_block;                               /* per unitig id: the block whose value it takes */
} msgpu_uf_tables;
/* mmap + one tokenising thread per chunk (as msgpu_parse_paf).  A line the stage rejects -- an empty file, a blank line,
 * fewer than 7 fields (MSGPU_E_FORMAT), an empty column 0 (MSGPU_E_FORMAT), column 1/2/3/6 not a decimal integer of
 * int32 range or a negative column 1/2/3, qend > the block's qlen (MSGPU_E_NUMBER) -- fails the parse with *err_line =
 * its 1-based number (1 for an empty file). */
int         msgpu_uf_parse(const char *path, msgpu_uf **out, uint64_t *err_line);
void        msgpu_uf_free(msgpu_uf *u);
int         msgpu_uf_get_tables(const msgpu_uf *u, msgpu_uf_tables *out);
const char *msgpu_uf_unitig_name(const msgpu_uf *u, uint32_t id);
const char *msgpu_uf_read_name(const msgpu_uf *u, uint32_t id);
uint32_t    msgpu_uf_unitig_id(const msgpu_uf *u, const char *name); /* 0xffffffff: no line names it */
/* numpy.percentile(values, [25, 75]) (linear method) and q3 + 1.5 * (q3 - q1), bit for bit; n >= 1 (host) */
int msgpu_uf_quartiles(const uint32_t *values, size_t n, double *q1, double *q3, double *upper);

/* device = HIP ordinal (MSGPU_E_NODEVICE without a GPU) */
int         msgpu_uf_create(int device, msgpu_ufctx **out);
void        msgpu_uf_destroy(msgpu_ufctx *ctx);
const char *msgpu_uf_last_error(const msgpu_ufctx *ctx);
uint64_t    msgpu_uf_error_line(const msgpu_ufctx *ctx); /* after MSGPU_E_IDS: 1-based PAF line of the first block whose unitig the FASTA lacks */
#define MSGPU_UF_PACKED 1u /* gather from the 2-bit store (msgpu_seq_pack_store) instead of the byte-per-base one */
typedef struct msgpu_uf_stats {
  uint64_t n_lines, n_blocks, n_ids, n_outliers, n_rescued, n_fragments, n_records, bases, text_bytes;
  uint32_t n_wave, n_group, n_giant, pad; /* pass-1 blocks per width class                                    */
  double   q1, q3, upper;
  float    load_ms;    /* host: FASTA parse + upload + descriptions (wall)                                   */
  float    upload_ms;  /* device: the PAF tables to HBM (events, as every *_ms below but plan_ms / wall_ms)   */
  float    pass1_ms;   /* block values, per-id values                                                        */
  float    pass2_ms;   /* outlier sweep: count + emit (plus the count read-back between them)                */
  float    plan_ms;    /* host: records, headers, gather plan                                                */
  float    gather_ms, format_ms, copy_ms;
  float    wall_ms;
  float    pad2;
} msgpu_uf_stats;
/* The whole stage on a parsed PAF: the unitigs are read as FASTA (first record of an id wins), the text of out.fa is kept
 * in the result.  MSGPU_E_IDS when a block names a unitig the FASTA lacks (msgpu_uf_error_line). Synchronous. */
int         msgpu_uf_run(msgpu_ufctx *ctx, const msgpu_uf *u, const char *unitigs_path, uint32_t flags, msgpu_uf_result **out);
int         msgpu_uf_result_stats(const msgpu_uf_result *r, msgpu_uf_stats *out);
const char *msgpu_uf_result_text(const msgpu_uf_result *r, uint64_t *len);
void        msgpu_uf_result_free(msgpu_uf_result *r);

/* ==== read scrubber: the pipeline's own step that cuts every long read into the stretches evidence covers ===============
 * (pipeline/scrubber_bfs.py).  Input: the anchor -> read PAF, the reads, and a read-to-read PAF
 * mapped once over all reads (the script maps every batch with minimap2; the stage uses the lines whose two reads are in
 * the batch, in file order).  The rules:
 *  1. anchor PAF, in line order: a line of one token is skipped, one of 2..8 fields is MSGPU_E_FORMAT; a line with
 *     col3 - col2 < 500 is skipped; a read (column 5) is a node from its first surviving line on (ids in that order, length
 *     = column 6 of that line); of several surviving lines of one (read, anchor) the first counts, with the read-side range
 *     (col7, col8); a chunk is a maximal run of counting lines with one column 0; a counting line joins its read to every
 *     read already in the chunk (an edge is added once) and a node's neighbours are ordered by when their edge was added;
 *  2. batches: breadth-first from the smallest remaining name outside the subset (bytewise order), nodes in discovery order
 *     until the subset holds subset_size nodes; a component that leaves it smaller merges into the next start; the centre of
 *     a closed batch is every subset node without a remaining neighbour outside the subset;
 *  3. read-to-read lines of a batch, in file order: skipped are lines of fewer than 6 fields, col0 == col5, a name that is
 *     not a node, col3 - col2 < 500; a line folds (col2, col3, strand) into the entry of (col0, col5) and (col7, col8,
 *     strand) into that of (col5, col0): the first line creates (S, E, D); a later (s, e, d) with d == D and (|S - e| < 500
 *     or |s - E| < 500) makes it (min(s, S), max(e, E), D).  Entries persist from batch to batch;
 *  4. per centre node: its entries' (S, E) and its anchor ranges sorted as pairs and merged left to right (a range joins
 *     the last covered one when cs <= e and s <= ce); covered range i is the record ">{read}_{i}" with the bases
 *     [max(cs, 200), min(ce, length - 200)], end inclusive, clipped to the record, in lines of 60.  The centre leaves the
 *     graph.  Records come out batch after batch, inside a batch by node id. */
typedef struct msgpu_scrub msgpu_scrub;           /* the two parsed PAFs (host)           */
typedef struct msgpu_scrub_plan msgpu_scrub_plan; /* the batches of rule 2 (host)         */
typedef struct msgpu_scrubctx msgpu_scrubctx;     /* a device context of the stage        */
typedef struct msgpu_scrub_result msgpu_scrub_result;
typedef struct msgpu_scrub_tables { /* views into a msgpu_scrub (valid while it lives)                                 */
  uint64_t        n_anchor_lines, n_ava_lines; /* lines of the two files                                                */
  uint64_t        n_hits, n_ava;               /* counting anchor lines; surviving read-to-read lines                   */
  uint32_t        n_nodes, n_anchors, n_chunks, pad;
  const int32_t  *node_length;                 /* per node: column 6 of its first surviving line                        */
  const uint32_t *node_line;                   /* per node: that line (0-based)                                         */
  const uint32_t *hit_node, *hit_anchor, *hit_line; /* per counting line, in line order                                 */
  const int32_t  *hit_s, *hit_e;               /* columns 7, 8                                                          */
  const uint32_t *chunk_first, *chunk_n;       /* per chunk: its counting lines [first, first + n)                      */
  const uint32_t *ava_a, *ava_b, *ava_strand, *ava_line; /* per surviving line: nodes of columns 0 / 5, strand id (0 '+',
                                                  1 '-', others from 2 in first-seen order), line (0-based)              */
  const int32_t  *ava_sa, *ava_ea, *ava_sb, *ava_eb; /* columns 2, 3, 7, 8                                             */
} msgpu_scrub_tables;
/* mmap + one tokenising thread per chunk of each file, then one pass in line order (first-seen ids, first-hit test,
 * chunks).  A line the script would stop on fails the parse with *err_line = its 1-based number and *err_file = 0 (anchor
 * PAF) or 1 (read-to-read PAF): 2..8 fields where 9 are read (MSGPU_E_FORMAT), an empty column 0 of an anchor line
 * (MSGPU_E_FORMAT), a column that is not a decimal integer of int32 range (MSGPU_E_NUMBER; columns 2, 3, 7, 8 without
 * sign, column 6 with an optional '-'), a node whose length is below 200 (MSGPU_E_NUMBER: its slice would end at a
 * negative index).  An anchor PAF without a node is MSGPU_E_FORMAT at line 1. */
int         msgpu_scrub_parse(const char *anchors_path, const char *ava_path, msgpu_scrub **out, uint64_t *err_line,
                              int *err_file);
void        msgpu_scrub_free(msgpu_scrub *s);
int         msgpu_scrub_get_tables(const msgpu_scrub *s, msgpu_scrub_tables *out);
const char *msgpu_scrub_node_name(const msgpu_scrub *s, uint32_t id);
uint32_t    msgpu_scrub_node_id(const msgpu_scrub *s, const char *name); /* 0xffffffff: not a node */
int         msgpu_scrub_name_order(const msgpu_scrub *s, uint32_t *out); /* the node ids sorted by name (n_nodes entries) */
/* Rule 2 on a graph in CSR form (row_off: n_nodes + 1 entries; a row's neighbours in insertion order) with by_name = the
 * node ids sorted by name.  MSGPU_E_LAYOUT when a batch closes with an empty centre (the script would build it again for
 * ever): *bad_node = the batch's first start.  Host only. */
typedef struct msgpu_scrub_plan_tables {
  uint32_t        n_batches, pad;
  const uint64_t *subset_off, *centre_off; /* n_batches + 1 entries each                                              */
  const uint32_t *subset;                  /* a batch's subset in the order its nodes were added                      */
  const uint32_t *centre;                  /* a batch's centre by ascending node id                                   */
  const uint32_t *start;                   /* per batch: its first start                                              */
} msgpu_scrub_plan_tables;
int  msgpu_scrub_plan_create(uint32_t n_nodes, const uint32_t *by_name, const uint64_t *row_off, const uint32_t *adj,
                             uint32_t subset_size, msgpu_scrub_plan **out, uint32_t *bad_node);
int  msgpu_scrub_plan_get(const msgpu_scrub_plan *p, msgpu_scrub_plan_tables *out);
void msgpu_scrub_plan_free(msgpu_scrub_plan *p);

/* device = HIP ordinal (MSGPU_E_NODEVICE without a GPU) */
int         msgpu_scrub_create(int device, msgpu_scrubctx **out);
void        msgpu_scrub_destroy(msgpu_scrubctx *ctx);
const char *msgpu_scrub_last_error(const msgpu_scrubctx *ctx);
uint64_t    msgpu_scrub_error_line(const msgpu_scrubctx *ctx); /* after MSGPU_E_IDS: 1-based anchor PAF line of the first node the reads file lacks */
#define MSGPU_SCRUB_SUBSET 60000u /* the script's subset_size */
typedef struct msgpu_scrub_stats {
  uint64_t n_nodes, n_hits, n_pairs, n_edges, n_ava, n_batches, n_subset_total, n_intervals, n_records, bases,
      text_bytes;
  float load_ms;    /* host: reads parse + upload (wall)                                                              */
  float graph_ms;   /* device: pairs, two sorts, CSR, its copy back (events, as fold / union / gather / format / copy) */
  float batch_ms;   /* host: rule 2                                                                                   */
  float fold_ms;    /* device: the sort of the directed entries and one launch pair per batch                         */
  float union_ms;   /* device: intervals, segmented sort, count, scan, emit, the ranges' copy back                    */
  float plan_ms;    /* host: records, headers, gather plan                                                            */
  float gather_ms, format_ms, copy_ms;
  float wall_ms;
} msgpu_scrub_stats;
/* The whole stage on the parsed PAFs: the reads are a FASTA when reads_path ends in "fa" or "fasta", else a FASTQ (first
 * record of a name wins); the text of the output is kept in the result.  MSGPU_E_IDS when a node is missing from the reads
 * (msgpu_scrub_error_line), MSGPU_E_LAYOUT for a batch with an empty centre (msgpu_scrub_last_error names its start read).
 * Synchronous. */
int         msgpu_scrub_run(msgpu_scrubctx *ctx, const msgpu_scrub *s, const char *reads_path, uint32_t subset_size,
                            msgpu_scrub_result **out);
int         msgpu_scrub_result_stats(const msgpu_scrub_result *r, msgpu_scrub_stats *out);
const char *msgpu_scrub_result_text(const msgpu_scrub_result *r, uint64_t *len);
/* the read graph the device built: row_off (n_nodes + 1 entries) and the neighbours in insertion order */
int         msgpu_scrub_result_graph(const msgpu_scrub_result *r, const uint64_t **row_off, const uint32_t **adj);
void        msgpu_scrub_result_free(msgpu_scrub_result *r);

/* ==== k-mer abundance filter: the pipeline's first step, "K-mer Filtering of Illumina Reads" =============================
 * (pipeline/pipeline.sh:136-151: jellyfish count -C / histo, the pipeline's setAbundanceThresholdFromHisto.py, jellyfish
 * dump -L, bbduk hdist=0).  Input: k (1..64) and two FASTQ files of equally many records; record i
 * of the one and record i of the other are a pair.  The threshold rule is pinned to the reference script (its outputs
 * recorded under tests/golden/kmer_filter); counting and filtering are defined by these rules:
 *  1. FASTQ: four lines per record, only '\n' ends a line, a last line without '\n' counts.  Line 1 starts with '@', line 3
 *     with '+', lines 2 and 4 have the same number of bytes (0 is allowed).  Anything else is MSGPU_E_FORMAT with the file
 *     (0 / 1) and the smallest offending 1-based line; a file that ends inside a record is one at the first missing line; two
 *     files of different record counts are one in the shorter file, at its first missing line.  File 0 is judged first.
 *  2. k-mers: a window is k consecutive bytes of a line 2, all of them in ACGTacgt (case folded); any other byte breaks the
 *     windows that hold it.  A=0, C=1, G=2, T=3, first base most significant, a 2k-bit unsigned number; the canonical k-mer
 *     of a window is the smaller of that number and the number of its reverse complement (jellyfish's -C).  A read shorter
 *     than k has no window.
 *  3. counts: count(x) = windows of both files whose canonical k-mer is x.  Exact (the "classic approach" pipeline.sh keeps
 *     as a comment; the --bf-size run it uses approximates the same table above abundance 1).
 *  4. histogram: row (a, f): f distinct canonical k-mers have count a, 1 <= a <= 10000; one row a = 10001 holds every k-mer
 *     with a count above 10000 (jellyfish histo's default --high); rows with f = 0 are left out; text "a f\n", ascending.
 *  5. threshold: what the script prints for that histogram and total = sum of f over the rows with a != 1:
 *     q1_th = round((total + 1) * 0.25), q3_th = round((total + 1) * 0.75), half to even; rows with a > 1 in order, a running
 *     sum of f; q1 = a of the first row where the sum reaches q1_th, q3 = a of the first LATER row where it reaches q3_th (the
 *     row that sets q1 never sets q3); upper = q3 + 2 * (q3 - q1).  q3 never set (the script prints a number <= 0) or no row
 *     besides a = 1 (the script dies) is MSGPU_E_LAYOUT, "degenerate histogram".  Whenever q3 is set, q3 > q1 >= 2, hence
 *     upper >= 5: the count pass discards k-mers with a count below 5 once they are in the histogram.
 *  6. abundant set: the canonical k-mers with count >= upper (jellyfish dump -L).
 *  7. verdict: pair i is dropped when read 1 or read 2 has at least one window whose canonical k-mer is in the abundant set
 *     (bbduk's hdist=0).  Surviving pairs are written in input order, a record as its four input lines byte for byte, each
 *     ended by '\n'.
 *  8. report: "abundance threshold for k-mer filtering:  <upper>\n" (two blanks, as the pipeline's echo writes it).
 * On any error nothing is produced.  Limits: a file below 2^40 bytes and 2^32 records; both files, the partition buffers and
 * the outputs are resident together, otherwise MSGPU_E_NOMEM with the sizes in msgpu_kf_last_error. */
typedef struct msgpu_kfctx msgpu_kfctx; /* a device context of the stage */
typedef struct msgpu_kf_result msgpu_kf_result;
/* Rule 5 on histogram rows (host only, works without a device).  MSGPU_E_LAYOUT for a degenerate histogram: *q1, *q3 and
 * *upper then hold what the script would have computed (0 where it set nothing). */
int         msgpu_kf_threshold(const uint64_t *abundance, const uint64_t *frequency, size_t n, int64_t *q1, int64_t *q3,
                               int64_t *upper);
/* device = HIP ordinal (MSGPU_E_NODEVICE without a GPU) */
int         msgpu_kf_create(int device, msgpu_kfctx **out);
void        msgpu_kf_destroy(msgpu_kfctx *ctx);
const char *msgpu_kf_last_error(const msgpu_kfctx *ctx);
uint64_t    msgpu_kf_error_line(const msgpu_kfctx *ctx); /* after MSGPU_E_FORMAT: the 1-based line */
int         msgpu_kf_error_file(const msgpu_kfctx *ctx); /* after MSGPU_E_FORMAT / MSGPU_E_IO: 0 or 1 */
typedef struct msgpu_kf_stats {
  uint64_t n_pairs, n_pairs_out; /* pairs read; pairs that survive                                                      */
  uint64_t n_windows;            /* rule 2, both files                                                                   */
  uint64_t n_distinct;           /* distinct canonical k-mers                                                            */
  uint64_t n_candidates;         /* of those, count >= 5: what is kept until the threshold is known                      */
  uint64_t n_abundant;           /* rule 6                                                                               */
  uint64_t n_hist_rows;
  uint64_t largest_partition;    /* keys in the largest partition                                                        */
  uint64_t bytes_in[2], bytes_out[2];
  int64_t  q1, q3, upper;
  uint32_t k, n_partitions;
  float load_ms;    /* host: both files mmap -> page-locked ring -> device (wall)                                        */
  float records_ms; /* line starts and the format check of both files (wall; device work and four small copies)          */
  float bins_ms;    /* device, by events from here on: windows per hash bin                                              */
  float extract_ms; /* keys of a partition, summed over the partitions (as sort / runs / hist / select)                  */
  float sort_ms, runs_ms, hist_ms;
  float select_ms;  /* candidates per partition; the abundant set, its sort and its table                                */
  float verdict_ms;
  float output_ms;  /* lengths, scan, record copy, both files                                                            */
  float copy_ms;    /* outputs, verdicts and the abundant set back to the host                                           */
  float wall_ms;
} msgpu_kf_stats;
/* The whole stage.  flags must be 0.  budget_bytes bounds the partition buffers (two key buffers and the run lengths: 20
 * bytes per key for k <= 32, 36 above); 0 = half of the device memory that is free once both files are resident and the
 * outputs are set aside.  The keys are cut into the smallest number of partitions (by a hash of the canonical key, so every
 * k-mer lies in exactly one and the result does not depend on the number) whose largest stays within the budget and below
 * 2^31 keys.  Synchronous; the outputs' text is kept in the result. */
int         msgpu_kf_run(msgpu_kfctx *ctx, int k, const char *path_a, const char *path_b, uint32_t flags,
                         uint64_t budget_bytes, msgpu_kf_result **out);
/* A short-read pair that stays in device memory: both files' bytes, their line starts, rule 1 checked --
 * what msgpu_kf_run leaves on the device in front of its count.  It is opened through a filter context, which takes the
 * error (msgpu_kf_last_error / _error_file / _error_line as after msgpu_kf_run; two files of different record counts are
 * accepted here and are msgpu_kf_run_pair's MSGPU_E_FORMAT), lives on that context's device until msgpu_pair_close, and
 * may outlive the context.  Runs read it and never write into it: any number of runs of the filter and of the unitig
 * stage (msgpu_ug_run_pair), at any k and in any order, each give what the run by files gives.  A pair on another device
 * than the running context's is MSGPU_E_ARG.  Budgets: a run on a pair counts the pair as resident -- "0 = what is free"
 * is measured with the pair in place -- and sets nothing aside for outputs beyond what it writes itself (the filter: its
 * two output texts; the unitig stage: nothing of the filter's).  msgpu_kf_run is msgpu_kf_open_pair, msgpu_kf_run_pair,
 * msgpu_pair_close; load_ms and records_ms of a run on a pair are 0, msgpu_kf_run fills them from the opening. */
typedef struct msgpu_pair msgpu_pair;
int         msgpu_kf_open_pair(msgpu_kfctx *ctx, const char *path_a, const char *path_b, msgpu_pair **out);
void        msgpu_pair_close(msgpu_pair *pair);
int         msgpu_kf_run_pair(msgpu_kfctx *ctx, int k, const msgpu_pair *pair, uint32_t flags, uint64_t budget_bytes,
                              msgpu_kf_result **out);
int         msgpu_kf_result_stats(const msgpu_kf_result *r, msgpu_kf_stats *out);
int         msgpu_kf_result_histogram(const msgpu_kf_result *r, const uint64_t **abundance, const uint64_t **frequency,
                                      uint64_t *n);
/* rule 6, ascending: the key's upper and lower 64 bits (upper = 0 for k <= 32) and its count */
int         msgpu_kf_result_abundant(const msgpu_kf_result *r, const uint64_t **key_hi, const uint64_t **key_lo,
                                     const uint32_t **count, uint64_t *n);
int         msgpu_kf_result_verdicts(const msgpu_kf_result *r, const uint8_t **verdict, uint64_t *n); /* 1 = dropped */
#define MSGPU_KF_TEXT_OUT_A 0  /* the surviving records of file 0 */
#define MSGPU_KF_TEXT_OUT_B 1
#define MSGPU_KF_TEXT_REPORT 2 /* rule 8 */
#define MSGPU_KF_TEXT_HISTO 3  /* rule 4 */
#define MSGPU_KF_TEXT_KMERS 4  /* rule 6 as ">count\nKMER\n" records (jellyfish dump's format), ascending; built on first use */
const char *msgpu_kf_result_text(msgpu_kf_result *r, int which, uint64_t *len);
void        msgpu_kf_result_free(msgpu_kf_result *r);

/* ==== short-read unitig assembly: the step behind the k-mer filter, `abyss-pe ... unitigs` and the awk cut at MINLENGTH ===
 * (pipeline/pipeline.sh).  ABySS is not part of the reference tree, so the stage is defined by these
 * rules and checked against their plain-Python restatement (tests/ug_oracle.py), not against ABySS.  Parameters: k (2..64,
 * or 2..128 after msgpu_ug_set_wide), min_count (>= 1, default 2), trim (>= 0, default k: the longest tip, in k-mers), min_length (default 500).
 *  1. input: one or two FASTQ files.  The FASTQ rules and the window rules are rules 1 and 2 of the k-mer abundance filter,
 *     word for word, error code, file and line included.  The files are not pairs: their record counts may differ and the
 *     second path may be NULL.  count(x) = windows of all files whose canonical k-mer is x, exact.
 *  2. solid set S = the canonical k-mers with count >= min_count.
 *  3. oriented graph: every k-base string s whose canonical form is in S is an oriented node; s and rc(s) are two nodes of
 *     one k-mer, or one node if s is its own reverse complement.  succ(s) = { s[1:]+c : c in ACGT, canon(s[1:]+c) in S },
 *     pred(s) = { c+s[:-1] : c in ACGT, canon(c+s[:-1]) in S }.
 *  4. tip removal, in rounds on a snapshot of S.  The limits are 1, 2, 4, ... (doubling, every value below trim), then trim;
 *     each limit runs once, after that the round at trim repeats until a round removes nothing; trim = 0: no round.  In a
 *     round, for every oriented node s with pred(s) empty: path = [s], then repeat: if |succ(last)| != 1 stop, no tip; let t
 *     be the one successor; if |pred(t)| >= 2 the path is a tip, stop; if |path| = limit stop, no tip; else append t.  All
 *     k-mers of all tips of a round leave S together when the round ends.  Islands (dead at both ends) stay.  Each round's
 *     (limit, k-mers removed) is reported.
 *  5. unitigs: s -> t is joined iff succ(s) = {t}, pred(t) = {s}, neither s nor t is its own reverse complement and
 *     canon(s) != canon(t): no self-loop and no hairpin is ever joined.  Unitigs are the maximal chains of joined nodes;
 *     every k-mer of S lies in exactly one.  Every unitig exists as two mirror chains, which these rules make distinct (a
 *     one-node chain of a self-complementary k-mer exists once).  Linear chain: the one whose first k-mer, as a 2k-bit
 *     number, is smaller than its mirror's first k-mer is emitted (no tie is possible).  Cycle: it starts at the smallest
 *     oriented node among the cycle and its mirror and goes round once: n k-mers give n + k - 1 bases, the closing join is
 *     not written.  Sequence = the first k-mer and the last base of every further node, upper case.  coverage = sum of
 *     count over its k-mers (64 bits).
 *  6. output: the unitigs ascending by the first k-mer of the emitted orientation; id = rank in that order, over all
 *     unitigs, before any cut.  A record is ">id length coverage\n", the sequence on one line, "\n" (ABySS's header shape;
 *     the pipeline's awk reads field 2).  Two texts: all records, and the records with length >= min_length, ids unchanged
 *     (the pipeline's ${NAME}-unitigs.l500.fa).
 *  7. limits, each an error and never a fault: fewer than 2^31 solid k-mers; the file limits of the k-mer filter; everything
 *     resident together, else MSGPU_E_NOMEM naming the sizes.  On any error nothing is produced.
 *  8. the mask (msgpu_ug_run_pair): the stage on a pair with the mask m (a byte per pair, 1 = dropped, what
 *     msgpu_kf_result_verdicts returns) gives the result of msgpu_ug_run on the two files that hold the records i with
 *     m[i] = 0, in order: both texts, the unitig table, the rounds, n_windows, n_distinct, n_solid, n_solid_trimmed, the unitig
 *     counts and longest_chain.  n_records and bytes_in are the pair's own.  A dropped pair's two reads have the length 0 for
 *     every kernel that forms windows.  With a mask both files hold n_pairs records, else MSGPU_E_ARG.
 *  9. bubble popping, on request (msgpu_ug_set_bubbles).  The parameter is bubble >= 0, the longest branch in k-mers; 0 means
 *     off, and rules 1-8 alone apply; a SNP makes branches of k k-mers, so values from k upwards are useful; values above
 *     4096 are MSGPU_E_ARG.
 *     (a) Simple branch.  All degrees are taken in the snapshot S of the round.  Let u be an oriented node with
 *         |succ(u)| >= 2, and b in succ(u).  If |pred(b)| != 1 there is no branch.  path = [b], then repeat: if
 *         |succ(last)| != 1 there is no branch; let t be the one successor; if |pred(t)| >= 2 the branch is path and its
 *         merge is t; otherwise, if |path| = bubble there is no branch; otherwise append t.  This is the tip walk of rule 4
 *         with a fork in front of it.  A successor of u that is itself a merge (|pred| >= 2) is no branch.
 *     (b) Bubble.  A bubble is a fork u, a merge t, and the >= 2 simple branches of u whose merge is t.  It must have
 *         canon(u) != canon(t): a bubble whose fork and merge are one k-mer is never popped (a palindromic passage).  The
 *         mirror of the bubble (u, t) is the bubble (rc(t), rc(u)).  A bubble is judged once, from the side whose fork is the
 *         smaller 2k-bit string: from u iff u < rc(t).
 *     (c) Winner.  The winner is the branch with the greatest mean count: branch A beats branch B iff
 *         sum(A) len(B) > sum(B) len(A), sum = the sum of count over the branch's k-mers, the products in 64 bits (the cap of
 *         4096 keeps them below 2^56).  Among equals, the branch entered from the judging fork by the smaller base c wins.
 *         Every k-mer of every other branch of the bubble leaves S.  One fork may hold several bubbles (different merges);
 *         each is judged alone.
 *     (d) Rounds.  A bubble round judges all bubbles on a snapshot; all losers leave together when the round ends.  A
 *         branch's inner nodes have in- and out-degree 1, so each k-mer lies in at most one branch of one bubble or its
 *         mirror, and no round removes a winner.  The neighbour bytes are refreshed behind a round as behind a tip round.
 *     (e) Order of the phases.  Rule 4 runs as it is.  Then a bubble phase: rounds repeat until a round removes nothing (that
 *         last round is recorded too).  If the bubble phase removed nothing in total, or trim = 0, cleaning is done.
 *         Otherwise a tip phase runs: the round at trim alone, repeated until it removes nothing; if it removed nothing,
 *         cleaning is done, otherwise the next bubble phase runs.  Rules 5-8 then run on what is left; n_solid_trimmed is
 *         what cleaning leaves.
 *     (f) Not done: complex bubbles (overlapping variants whose branches fork again or merge at different nodes) and
 *         zero-length branches are left alone, and there is no erosion.
 * 10. the unitig graph as GFA 1, on request (msgpu_ug_set_graph).  It is off by default, and with it off every output, table,
 *     count and kernel launch of the stage is what rules 1-9 make it.  The rule is defined on what rules 1-9 leave.
 *     (a) Oriented unitigs.  Unitig i (its id is its rank, rule 6) exists as i+ and i-: i+ is the emitted chain and i- is its
 *         mirror.  A unitig that is one self-complementary k-mer exists as i+ only.  first(x) and last(x) are the first and
 *         the last oriented node of the oriented unitig x.
 *     (b) Adjacencies.  For every oriented unitig x and every t in succ(last(x)) (rule 3, on the cleaned set) there is an
 *         adjacency x -> y with first(y) = t.  Such a y always exists: an edge that rule 5 did not join ends at a node
 *         without a joined predecessor.  The closing join of a cycle is the adjacency i+ -> i+.
 *     (c) Mirror.  x -> y and y' -> x' are one link; ' flips the orientation.  As tuples (from id, from orientation, to id,
 *         to orientation) with + < -, the smaller of the two is written.  Equal tuples (a hairpin i+ -> i-) are written
 *         once.  A unitig that exists as i+ only has no i-, so an adjacency with such a unitig at either end has no mirror:
 *         it is written as it is and is counted with the self-mirrored links.  (A reader of GFA takes the mirror of
 *         x+ -> i+ to be i- -> x-, so the adjacency i+ -> x- needs a line of its own.)
 *     (d) Order.  The links are written ascending by that tuple.
 *     (e) Text, GFA 1.  The header "H\tVN:Z:1.0\n"; one line per unitig in id order,
 *         "S\t<id>\t<sequence>\tLN:i:<length>\tKC:i:<coverage>\n", where sequence, length and coverage are exactly those of
 *         the FASTA record (rule 6); one line per link, "L\t<from>\t<+|->\t<to>\t<+|->\t<k-1>M\n".  All unitigs are
 *         written, with no length cut: links to short unitigs would otherwise dangle.
 *     (f) Limits, each an error and never a fault.  Rule 7's bound of fewer than 2^31 solid k-mers makes the tuple fit 64 bits
 *         (31 + 1 + 31 + 1); fewer than 2^32 links; device memory as in rule 7, MSGPU_E_NOMEM naming the sizes.  The counts
 *         obey adjacencies = 2 links - self-mirrored links. */
typedef struct msgpu_ugctx msgpu_ugctx; /* a device context of the stage */
typedef struct msgpu_ug_result msgpu_ug_result;
typedef struct msgpu_ug_params {
  int32_t  k;
  uint32_t min_count;
  int32_t  trim; /* -1: k */
  uint32_t min_length;
} msgpu_ug_params;
int         msgpu_ug_create(int device, msgpu_ugctx **out); /* MSGPU_E_NODEVICE without a GPU */
void        msgpu_ug_destroy(msgpu_ugctx *ctx);
const char *msgpu_ug_last_error(const msgpu_ugctx *ctx);
uint64_t    msgpu_ug_error_line(const msgpu_ugctx *ctx); /* after MSGPU_E_FORMAT: the 1-based line */
int         msgpu_ug_error_file(const msgpu_ugctx *ctx); /* after MSGPU_E_FORMAT / MSGPU_E_IO: 0 or 1 */
typedef struct msgpu_ug_stats {
  uint64_t n_records[2];
  uint64_t n_windows, n_distinct;
  uint64_t n_solid, n_solid_trimmed; /* rule 2; what rule 4 leaves                                                        */
  uint64_t n_unitigs, n_unitigs_kept, n_cycles;
  uint64_t longest_chain;            /* k-mers of the longest unitig                                                       */
  uint64_t largest_partition;
  uint64_t n_lost_publications;      /* scalar read-backs that had to fall back to a copy                                  */
  uint64_t bytes_in[2], bytes_out[2]; /* bytes_out: the all text, the cut text                                            */
  uint32_t k, min_count, trim, min_length;
  uint32_t n_tip_rounds, doubling_rounds, n_partitions, reserved;
  float load_ms, records_ms;         /* host wall, as msgpu_kf_stats                                                       */
  float bins_ms, extract_ms, sort_ms, runs_ms, select_ms; /* the count, device by events from here on                     */
  float adjacency_ms;                /* the neighbour bytes: the first fill and the refresh behind every tip round         */
  float tips_ms;                     /* the tip rounds themselves (walk, apply)                                            */
  float next_ms;                     /* rule 5's joins                                                                     */
  float doubling_ms;                 /* pointer doubling, the cycles' minima included                                      */
  float order_ms;                    /* heads, their sort, the unitig table, coverage                                      */
  float write_ms;                    /* the bases                                                                          */
  float copy_ms;                     /* tables and text back to the host                                                   */
  float host_ms;                     /* host: headers, offsets, the cut text (wall)                                        */
  float wall_ms;
} msgpu_ug_stats;
typedef struct msgpu_ug_round {
  uint32_t limit, reserved;
  uint64_t removed;
  float    tips_ms, adjacency_ms; /* device, by events */
} msgpu_ug_round;
typedef struct msgpu_ug_unitig { /* in output order: entry i is the unitig with id i */
  uint64_t length, coverage;
  uint64_t first_hi, first_lo;   /* its first k-mer (upper half 0 for k <= 32; above k = 64 its low 128 bits) */
  uint64_t offset;               /* of its sequence in the all text */
  uint32_t cyclic, reserved;
} msgpu_ug_unitig;
/* The whole stage.  path_b may be NULL.  flags must be 0.  budget_bytes bounds the count's partition buffers as in
 * msgpu_kf_run.  Synchronous; both texts are kept in the result. */
int         msgpu_ug_run(msgpu_ugctx *ctx, const msgpu_ug_params *params, const char *path_a, const char *path_b, uint32_t flags,
                         uint64_t budget_bytes, msgpu_ug_result **out);
/* The stage on a pair opened by msgpu_kf_open_pair (see there).  dropped: n_pairs bytes on the host, copied to the device
 * once, or NULL to keep every record (n_pairs is then ignored); rule 8.  msgpu_ug_run is open, this, close. */
int         msgpu_ug_run_pair(msgpu_ugctx *ctx, const msgpu_ug_params *params, const msgpu_pair *pair, const uint8_t *dropped,
                              uint64_t n_pairs, uint32_t flags, uint64_t budget_bytes, msgpu_ug_result **out);
int         msgpu_ug_result_stats(const msgpu_ug_result *r, msgpu_ug_stats *out);
int         msgpu_ug_result_rounds(const msgpu_ug_result *r, const msgpu_ug_round **rounds, uint64_t *n);
int         msgpu_ug_result_unitigs(const msgpu_ug_result *r, const msgpu_ug_unitig **unitigs, uint64_t *n);
/* Rule 9.  msgpu_ug_set_bubbles sets the parameter on the context for every later msgpu_ug_run / msgpu_ug_run_pair, until it is
 * set again; 0 switches it off (what a new context has).  Above MSGPU_UG_BUBBLE_MAX: MSGPU_E_ARG, the previous value stays
 * and msgpu_ug_last_error names the value.  With the feature off msgpu_ug_result_bubbles gives zeros and an empty table.
 * msgpu_ug_result_rounds keeps the tip rounds only, those of later tip phases included (n_tip_rounds counts them). */
#define MSGPU_UG_BUBBLE_MAX 4096u
typedef struct msgpu_ug_bubble_stats {
  uint32_t bubble, n_phases, n_rounds, reserved; /* the parameter; bubble phases; bubble rounds over all phases            */
  uint64_t n_bubbles, n_branches_removed, n_kmers_removed;
  uint64_t max_forks;                            /* the largest fork list of a round                                       */
  float    forks_ms, walk_ms;                    /* device, by events: the fork lists; the walks and their apply           */
  float    adjacency_ms, reserved2;              /* the neighbour bytes behind the bubble rounds                           */
} msgpu_ug_bubble_stats;
typedef struct msgpu_ug_bubble_round {
  uint32_t after_tip_rounds, reserved; /* entries of the tip-round table that precede this round */
  uint64_t forks, bubbles, branches_removed, removed;
  float    forks_ms, walk_ms;          /* device, by events */
} msgpu_ug_bubble_round;
int         msgpu_ug_set_bubbles(msgpu_ugctx *ctx, uint32_t bubble);
int         msgpu_ug_result_bubbles(const msgpu_ug_result *r, msgpu_ug_bubble_stats *out, const msgpu_ug_bubble_round **rounds,
                                    uint64_t *n);
/* Rule 10.  msgpu_ug_set_graph switches the unitig graph on (on != 0) or off (0, what a new context has) for every later
 * msgpu_ug_run / msgpu_ug_run_pair on the context, until it is set again.  With it off msgpu_ug_result_links gives zeros and
 * an empty table, and msgpu_ug_result_text has no MSGPU_UG_TEXT_GFA ("" and length 0, as for any unknown text). */
typedef struct msgpu_ug_link { /* in rule 10 (d)'s order */
  uint32_t from, to;           /* unitig ids */
  uint8_t  from_rev, to_rev;   /* 0: +, 1: - */
  uint16_t reserved;
} msgpu_ug_link;
typedef struct msgpu_ug_graph_stats {
  uint64_t n_links;                    /* L lines written                                                                  */
  uint64_t n_adjacencies;              /* oriented adjacencies seen, rule 10 (b): 2 n_links - n_self_mirror                 */
  uint64_t n_self_mirror;              /* links that stand for themselves, rule 10 (c)                                     */
  uint64_t n_dead_ends;                /* oriented unitig ends without a link                                              */
  uint64_t gfa_bytes;                  /* bytes of the GFA text                                                            */
  float    links_ms, sort_ms, text_ms; /* device, by events: the links; their sort; line lengths, offsets and the text     */
  float    reserved;
} msgpu_ug_graph_stats;
int         msgpu_ug_set_graph(msgpu_ugctx *ctx, int on);
/* k up to 128, on request.  msgpu_ug_set_wide switches the wide keys on (on != 0) or off (0, what a new context has) for every
 * later msgpu_ug_run / msgpu_ug_run_pair on the context, until it is set again.  Off: k above 64 is MSGPU_E_ARG ("k = 65 is
 * outside 2..64"), and every error, output, table, count and kernel launch is what it was.  On: the upper bound of k is 128
 * (k = 129 is MSGPU_E_ARG naming the figure); k <= 64 runs what it runs with the switch off and gives the same bytes;
 * k = 65..96 runs on keys of three 64-bit words, k = 97..128 on keys of four.  Rules 1-10 hold as they stand.
 * msgpu_ug_result_first_kmers gives the whole first k-mer of every unitig at any k: *words holds *words_per_kmer words per
 * unitig, least significant first, for the *n unitigs in output order; *words_per_kmer is 1 for k <= 32, 2 for k <= 64, 3 for
 * k <= 96 and 4 above.  The array lives as long as the result.  msgpu_ug_result_peak_bytes gives the most device memory the
 * run's own arena held at once, in bytes (the files of a pair are the pair's and are not counted; 0 for NULL). */
int         msgpu_ug_set_wide(msgpu_ugctx *ctx, int on);
int         msgpu_ug_result_first_kmers(const msgpu_ug_result *r, const uint64_t **words, uint32_t *words_per_kmer, uint64_t *n);
uint64_t    msgpu_ug_result_peak_bytes(const msgpu_ug_result *r);
int         msgpu_ug_result_links(const msgpu_ug_result *r, msgpu_ug_graph_stats *out, const msgpu_ug_link **links, uint64_t *n);
#define MSGPU_UG_TEXT_ALL 0 /* every record */
#define MSGPU_UG_TEXT_CUT 1 /* the records with length >= min_length */
#define MSGPU_UG_TEXT_GFA 2 /* rule 10 (e); only after msgpu_ug_set_graph(ctx, 1) */
const char *msgpu_ug_result_text(const msgpu_ug_result *r, int which, uint64_t *len);
void        msgpu_ug_result_free(msgpu_ug_result *r);

/* ---- unitig-to-read mapping (the pipeline's four minimap2 calls) ------------------------------
 * Every record of a query file is mapped onto every record of a target file by minimizer seeds and a chaining DP, and a PAF
 * is written.  minimap2 is not part of the reference tree: the stage is defined by the rules below, in integers only, and is
 * checked without tolerance against their restatement in plain Python (tests/map_oracle.py), not against minimap2.  Both files
 * go through msgpu_seq_parse_upload (FASTA or FASTQ, decided as msgpu_seq_parse decides; names are cut at the first
 * whitespace).  Parameters: k (4..32, default 15), w (1..64, 5), max_occ (>= 1, 200), max_gap (10000), bandwidth (2000),
 * max_pred (fixed at 64), min_score (100), min_count (3), exact (0 / 1), band (1..127, 64), ava (0 / 1).
 *  1. windows: the alphabet, case folding, 2-bit code, canonical key (min(fw, rc) as 2k-bit numbers) and the break at any
 *     other byte are those of the k-mer filter's rolling window (KfRoll).  A stretch is a maximal run of k-mer start
 *     positions without a break.  The strand bit of a position is 1 iff rc < fw.
 *  2. minimizers: h(i) = kf_hash(key(i)).  A window is w consecutive k-mer start positions inside one stretch; a stretch with
 *     fewer than w positions has none.  A window's minimizer is its position with the smallest (h, position).  A sequence's
 *     minimizers are the union over its windows, each position once.
 *  3. index: every target minimizer as (key, target record, position, strand).  A key with more than max_occ entries is left
 *     out whole; the number of keys and entries left out is reported.
 *  4. anchors: every query minimizer meets every index entry of its key.  Relative strand s = query strand ^ target strand,
 *     x = the target position, y = the query position if s = 0, else qlen - k - position (the position in the
 *     reverse-complemented query, so a collinear chain rises in both coordinates on both strands).  With ava the query file
 *     is the target file, and an anchor is kept only if the query record index is smaller than the target record index.  A
 *     group is (query record, target record, s); its anchors are ordered by (x, y); equal (x, y) cannot occur.
 *  5. chaining, per group over the anchors 0..n-1 in that order: f(i) = max(k, max over j in [max(0, i - 64), i) of
 *     f(j) + gain - pen), taken over the j with dx = x_i - x_j > 0, dy = y_i - y_j > 0, dx <= max_gap, dy <= max_gap and
 *     dd = |dx - dy| <= bandwidth; gain = min(dx, dy, k); pen = 0 if dd = 0, else (dd * k) / 100 + (floor(log2(dd)) >> 1)
 *     with integer division.  pred(i) is the j that gives the maximum, the largest such j on a tie; it is "none" when k
 *     alone is at least as good.
 *  6. chains: the anchors of a group are visited by (f descending, index ascending).  An unused anchor starts a chain; the
 *     chain follows pred over unused anchors and ends before the first used anchor u or at "none";
 *     score = f(start) - (f(u) if it ended at a used anchor, else 0); all its anchors become used.  The chain is emitted iff
 *     score >= min_score and it has at least min_count anchors.  A group with fewer than min_count anchors, or with
 *     n * k < min_score, can emit nothing and is dropped before the DP.
 *  7. figures of a chain with anchors a_0 < ... < a_{m-1} (rising x).  For each link i >= 1: c_i = min(dx, dy, k),
 *     lt_i = dx - c_i, lq_i = dy - c_i; the link's segment is target [x_i + k - c_i - lt_i, x_i + k - c_i) against the
 *     oriented query [y_i + k - c_i - lq_i, y_i + k - c_i); d_i = that pair's Levenshtein distance inside band with
 *     msgpu_edit_distance's semantics, min(distance, band + 1), over the bytes as the stores hold them (the oriented query
 *     of s = 1 is MSGPU_COPY_REVCOMP's: reversed, A <-> T and C <-> G in upper case, every other byte as it is); if
 *     lt_i = lq_i = 0 then d_i = 0; d_i is computed only in exact mode.  block = k + sum (c_i + max(lt_i, lq_i)).  Seed
 *     mode: matches = k + sum c_i.  Exact mode: matches = k + sum (c_i + max(lt_i, lq_i) - d_i), never negative because
 *     d_i <= max(lt_i, lq_i).  Target range [x_0, x_{m-1} + k).  Query range in forward coordinates: [y_0, y_{m-1} + k) for
 *     s = 0, [qlen - y_{m-1} - k, qlen - y_0) for s = 1.
 *  8. output: one line per chain: the twelve PAF columns ('+' / '-' in column 5, mapping quality 255), then cm:i:<anchors>,
 *     s1:i:<score> and, in exact mode, NM:i:<sum d_i>.  Lines are ordered by (query record, target record, strand, order of
 *     emission in the group).  On any error nothing is written.
 *  9. limits and batches.  Limits, each an error and never a fault: fewer than 2^31 index entries, anchors and segment pairs
 *     per batch, at most 2^30 distinct target keys; a record shorter than 2^31 bases, a file below 2^38; a group's n * k
 *     below 2^31.  Resident while the index lives (msgpu_map_index): the target store, its sketch and the index (sorted
 *     entries, distinct keys, counts, starts, hash table); resident for the whole run besides: the query store and sketch,
 *     the anchor count of every query minimizer and its 64-bit exclusive scan.  Everything whose size
 *     depends on the anchors exists per batch of consecutive query records (a group never spans two query records, and rule 8
 *     orders by query record first, so the batches' lines one behind the other are the PAF of the whole input): the anchors
 *     and their sort buffers, the groups, classes and lists, f, pred, the sort keys, the chains with their table and, in
 *     exact mode, the segment pairs, their distances and the oriented copies of the batch's query records (2 * their bases).
 *     msgpu_map_batch_bytes(params, anchors, query bases) bounds the device bytes of a batch.  The cut is greedy: with a(r),
 *     b(r) the anchors and bases of query record r, a batch starts at the first record not yet taken and takes consecutive
 *     records while msgpu_map_batch_bytes(params, sum a, sum b) <= budget and sum a < 2^31; it holds at least one record;
 *     records without anchors join the running batch; no query records, no batches.  budget_bytes > 0 is the budget of a
 *     batch (the resident part is not counted); 0 stands for the free device memory once the resident part is allocated (an
 *     eighth less, again and again, while the device cannot give the largest batch's bytes as one block).  A
 *     record that exceeds the budget on its own is MSGPU_E_NOMEM, one with 2^31 anchors or more MSGPU_E_ARG, naming the
 *     record, its anchors and the bytes against the budget.  Splitting one query record over ranges of targets, and
 *     splitting the index, are out of scope.
 * 10. the alignment of one segment pair, and cigar mode (cigar = 1, which needs exact = 1).  a is the target bytes, n of
 *     them, b the oriented query bytes, m of them, compared as the stores hold them (rule 7); ks = m - n; slide(i, k) is the
 *     largest i' >= i with a[i..i') == b[i+k..i'+k), i' <= n, i'+k <= m.  The table: G_0[0] = slide(0, 0) and nothing else
 *     is defined in row 0.  For e >= 1 and |k| <= e the candidates of cell (e, k) are X: G_{e-1}[k] + 1, valid iff
 *     G_{e-1}[k] is defined and < min(n, m - k); D (a target base without a query base): G_{e-1}[k+1] + 1, valid iff
 *     G_{e-1}[k+1] is defined and < n; I (a query base without a target base): G_{e-1}[k-1], valid iff it is defined and
 *     G_{e-1}[k-1] + k <= m.  x0(e, k) is the largest valid candidate (none: the cell is undefined), G_e[k] = slide(x0, k),
 *     and the cell's op is the first of X, D, I whose candidate is valid and equals x0.  d is the first e with
 *     G_e[ks] = n; the pair is capped when |ks| > band or no such e <= band exists, and then d_i = band + 1 as in rule 7.
 *     The script is read backwards from (d, ks): G_e[k] - x0 '=' columns lie behind the cell's op, which leads to
 *     (e-1, k) for X, (e-1, k+1) for D, (e-1, k-1) for I; row 0 ends the walk with G_0[0] leading '=' columns.  Only valid
 *     candidates enter: one that would step outside the matrix is no edit (rule 7's clamped recurrence may hold such
 *     values; they are harmless for the number, not for a script).  The script has exactly d columns that are not '=',
 *     every '=' column holds equal bytes and every X column unequal ones, and it consumes exactly n and m bytes.
 *     With cigar = 1 a chain's alignment is k '=' columns for anchor 0, then for every link in rising order the segment's
 *     script followed by c_i '=' columns (seed bases: '=' by rule 1's case folding even where the bytes differ in case);
 *     a link with lt_i = lq_i = 0 has no segment; a capped segment is written lt_i D then lq_i I, zero lengths left out;
 *     neighbouring runs of one letter are merged.  matches = the '=' columns, block = all columns, nm = block - matches.
 *     The line is the twelve columns, cm, s1, NM:i:<nm>, then cg:Z:<runs> in target-forward order, which is the oriented
 *     query's order on both strands.  The runs consume exactly t_end - t_start target bases and q_end - q_start query
 *     bases; for a chain without a capped segment matches is at least rule 7's exact-mode value (a segment has at least
 *     max(lt, lq) columns, d of them no '=').  Rule 9 with cigar = 1: msgpu_map_batch_bytes adds the slab of the scripts'
 *     tables (slots * (band + 1)^2 words, a constant number of slots that MSGPU_ALIGN_SLOTS=<n> lowers; no slab for a band
 *     of at most 31, whose tables all lie in LDS) to the fixed part
 *     and, per anchor, band + 1 words of script, the 64-bit offset, the script length, the class list entry, the '='
 *     columns behind the segment and the two column counts.  Without cigar every byte of every output is as before.
 * 11. end extension, on request (msgpu_map_set_extension).  The parameter is extend = E: 0 is off (a new context), 1..65535
 *     the longest flank on either sequence; E > 0 needs cigar = 1 (and so exact = 1), else the run is MSGPU_E_ARG naming
 *     both.  The penalty is a constant of the rule, P = 8.  (1) Flanks of a chain with anchors a_0..a_{m-1}, oq the oriented
 *     query of rule 7, tlen and qlen the lengths, rev byte reversal (no complement: oq is oriented already).  Right:
 *     A = target[t_end .. t_end + n), n = min(E, tlen - t_end); B = oq[yE .. yE + m), yE = y_{m-1} + k,
 *     m = min(E, qlen - yE).  Left: A = rev(target[x_0 - n .. x_0)), n = min(E, x_0); B = rev(oq[y_0 - m .. y_0)),
 *     m = min(E, y_0).  (2) The table is rule 10's on (A, n, B, m), rows e = 0..band: the same slide, the same three
 *     candidates with the same validity tests (only candidates that stay inside the matrix enter), the same tie order X, D,
 *     I.  Nothing of rule 10's end test is used: |m - n| may exceed the band and no row ends the table early.  (3) Every
 *     defined cell has x = G_e[k], y = x + k and score = x + y - P * e.  The end cell (e*, k*) is the one with the greatest
 *     score; on equal scores the smaller e wins, then the smaller |k|, then the negative k.  Cell (0, 0) always exists with
 *     score 2 * G_0[0] >= 0, so the end cell exists, and x* = y* = 0 means "no extension".  A row e with
 *     n + m - P * e <= the best score of the rows before it cannot win, nor can a later one: rows, the number of rows an
 *     end is charged with, is the first such e, or band + 1.  (4) The script is the walk back from (e*, k*) exactly as rule
 *     10 walks back from (d, ks): e* + 1 words, consuming exactly x* bytes of A and y* bytes of B, every '=' column equal
 *     and every X column unequal; a left flank's columns are written in reverse order.  (5) The chain: its runs are the left
 *     columns, rule 10's chain alignment, the right columns, neighbouring runs merged; t_start -= x*_L, t_end += x*_R; the
 *     oriented query range grows by y*_L and y*_R and rule 7 turns it into forward coordinates; matches, block and nm are
 *     counted on the columns; cm, s1, n_anchors, score, the chain's place in the output order and which chains exist are
 *     untouched.  The runs consume exactly the new target and query ranges.  (6) With E = 0 every byte is as before.  It
 *     follows that a flank whose shorter side matches the longer side's start without an edit is extended to that
 *     sequence's end: cell (0, 0) wins.  Rule 9 with E > 0: msgpu_map_batch_bytes_ext adds, per anchor, two ends' descriptors
 *     (24 bytes each), end cells (24 bytes each) and band + 1 script words each; the slab is cigar mode's.
 * 12. primaries, secondaries and mapping quality, on request (msgpu_map_set_ranking; off on a new context; it needs no other
 *     mode: seed, exact, cigar, ava and extend all combine with it).  The chains of one query record, over all targets and
 *     both strands, with their indices in output order (rule 8), are ranked among themselves.  For a chain c:
 *     len(c) = q_end - q_start of rule 7's forward query range, and ov(c, p) = max(0, min(q_end_c, q_end_p) -
 *     max(q_start_c, q_start_p)).  Rule 11 changes no rank: rule 12 reads the ranges as rule 7 leaves them, before any
 *     extension.  (1) Visiting order: by (score descending, output index ascending).  (2) A visited chain c is compared with
 *     the primaries visited before it, in visiting order: the first primary p with 2 * ov(c, p) > min(len(c), len(p)) makes c
 *     secondary with parent(c) = p; if there is none, c is primary and parent(c) = c.  The mask level is one half and the
 *     comparison is strict.  (3) Of a primary p: sub(p) is the greatest score among its secondaries, 0 if it has none;
 *     n_secondary(p) is the number of its secondaries s with 10 * score(s) >= 9 * score(p); both are 0 for a secondary.
 *     (4) mapq of a primary with s1 = score(p) > 0: (60 * (s1 - sub) * min(n_anchors, 10)) / (10 * s1), the products in 64
 *     bits, integer division, clamped to 0..60; 0 if s1 <= 0; 0 for a secondary.  (5) With ranking on column 12 is mapq and
 *     the tags are tp:A:P or tp:A:S, cm:i, s1:i, s2:i:<sub>, then NM and cg as before; line order, every other column, the
 *     chain table and the run tables are untouched.  (6) With ranking off every byte is as before: 255, no tp, no s2.
 *     (7) A query record's chains never span two batches (rule 9), so the rule runs per batch; parent is an index into the
 *     whole run's chain table (the batch's base is added on the device); with ranking on a run has fewer than 2^32 chains,
 *     else MSGPU_E_ARG.  msgpu_map_batch_bytes_rank bounds a batch (rule 9's cut and bytes_bound use it; it equals
 *     msgpu_map_batch_bytes_ext for ranking = 0): per anchor it adds 104 bytes (seven words of segment heads, numbers,
 *     starts, class flags and their scans, four of class lists and sort bounds, parent, n_secondary, a 64-bit sub, the row,
 *     two 64-bit sort keys, 12 bytes of the list class's stretch) and a fixed 24 * 256 bytes.  The mask level 1/2, the ratio
 *     0.9 and the mapq formula are choices modelled on minimap2's, unchecked on real reads.
 * 13. mates, on request (msgpu_map_set_mates(ctx, on, max_insert); off on a new context; it needs no other mode: seed, exact,
 *     cigar, extend and rank all combine with it; with ava it is MSGPU_E_ARG).  The query file is interleaved: records 2p and
 *     2p + 1 are mate 1 and mate 2 of pair p; the names are not compared; an odd number of query records is MSGPU_E_ARG naming
 *     the count.  max_insert is 1..2^31 - 1, default 1000.  The rule reads the chain table as the run leaves it, behind rule
 *     11's extension.  (1) Concordant: chain a of record 2p and chain b of record 2p + 1 are concordant iff they have the same
 *     target record, their strands differ, and with f the chain of strand 0 and r the chain of strand 1:
 *     f.t_start <= r.t_start, f.t_end <= r.t_end (the forward mate lies to the left and neither passes the other) and
 *     tl = r.t_end - f.t_start <= max_insert.  Either mate may be the forward one.  (2) Selection: among the concordant
 *     combinations of a pair one is selected: the greatest score(a) + score(b) (a 64-bit sum), then the smaller tl, then the
 *     smaller index of a, then the smaller index of b.  n_best is the number of concordant combinations whose sum equals the
 *     greatest sum, whatever their tl, clamped to 2^32 - 1.  (3) Rows, one per chain in output order, {mate, tlen, cls,
 *     n_best}: the two selected chains have cls = 1, mate = the other's index in the whole run's chain table, tlen = tl and
 *     the pair's n_best; every other chain has {0xffffffff, 0, 0, 0}.  (4) Counts (msgpu_map_mstats): the pairs of the input,
 *     proper pairs, ambiguous pairs (proper with n_best > 1), discordant pairs (chains on both mates, none concordant),
 *     single pairs (chains on one mate only), unmapped pairs, the pairs per kernel class, the largest pair in chains, the
 *     sum, minimum and maximum of tlen over the proper pairs (integers: no order reaches them) and the step's device time.
 *     (5) With mates on every line carries pr:A:P or pr:A:U behind s1:i (behind s2:i with ranking on); a P line also carries
 *     mi:i:<the mate's line, 0-based>, tl:i:<tlen>, nb:i:<n_best>; NM and cg follow as before; line order and every other
 *     column are untouched.  (6) With mates off every byte of every output is as before.  (7) Rule 9 with mates on: the unit
 *     of the greedy cut is the pair: a batch starts at an even record and holds whole pairs, a(p) = a(2p) + a(2p + 1) and
 *     likewise the bases; a pair that exceeds the budget on its own is MSGPU_E_NOMEM naming the pair; with mates on a run has
 *     fewer than 2^32 chains, else MSGPU_E_ARG.  msgpu_map_batch_bytes_mates bounds a batch (it equals
 *     msgpu_map_batch_bytes_rank for mates = 0): per anchor it adds 60 bytes (three words of segment heads, numbers and
 *     starts, the count of mate 1's chains, three words of class lists, 16 bytes of the pair's selection, the row) and a fixed
 *     12 * 256 bytes.  (8) Orientation FR only, the selection order and n_best are choices modelled on short-read mappers,
 *     unchecked on real reads. */
typedef struct msgpu_mapctx msgpu_mapctx; /* a device context of the stage */
typedef struct msgpu_map_result msgpu_map_result;
typedef struct msgpu_map_params {
  int32_t  k, w;
  uint32_t max_occ;
  int32_t  max_gap, bandwidth, max_pred, min_score, min_count;
  int32_t  exact, band, ava;
  int32_t  cigar; /* 0 / 1; 1 needs exact = 1 (rule 10) */
} msgpu_map_params;
void        msgpu_map_default_params(msgpu_map_params *p);
int         msgpu_map_create(int device, msgpu_mapctx **out); /* MSGPU_E_NODEVICE without a GPU */
void        msgpu_map_destroy(msgpu_mapctx *ctx);
const char *msgpu_map_last_error(const msgpu_mapctx *ctx);
typedef struct msgpu_map_chain { /* in output order: entry i is line i of the PAF */
  uint32_t query, target;  /* record indices */
  uint32_t strand, n_anchors;
  int32_t  score;
  uint32_t nm;             /* sum of d_i (exact mode, else 0) */
  uint32_t q_start, q_end, t_start, t_end;
  uint32_t matches, block;
} msgpu_map_chain;
typedef struct msgpu_map_stats {
  uint64_t n_records[2], n_bases[2], n_minimizers[2]; /* targets, queries */
  uint64_t n_keys, n_index_entries, n_keys_dropped, n_entries_dropped; /* rule 3 */
  uint64_t n_anchors, n_groups;
  uint64_t n_groups_kept, n_groups_small, n_groups_large; /* behind rule 6's pre-filter; at most 16 anchors; more */
  uint64_t largest_group;
  uint64_t n_chains, n_chains_below_score, n_chains_below_count, n_chains_cut; /* emitted; dropped; emitted and cut at a used anchor */
  uint64_t n_pairs, n_pairs_capped; /* exact mode: segment pairs, and those beyond the band */
  uint64_t n_lost_publications, bytes_out;
  uint64_t group_hist[16];          /* kept groups by floor(log2(anchors)), the last bin open */
  msgpu_map_params params;
  float load_ms;                    /* host wall: both files into their stores */
  float sketch_ms, sort_ms, table_ms, anchors_ms, group_ms, chain_ms, backtrack_ms, pairs_ms, distance_ms, copy_ms; /* device, by events */
  float host_ms;                    /* host: the lines (wall) */
  float wall_ms;
} msgpu_map_stats;
/* An upper bound on the device bytes that a batch of rule 9 with n_anchors anchors and n_query_bases bases of query records
 * allocates: a constant plus a multiple of each argument; n_query_bases counts only when params->exact is set.  A host
 * function without any device call. */
uint64_t    msgpu_map_batch_bytes(const msgpu_map_params *params, uint64_t n_anchors, uint64_t n_query_bases);
typedef struct msgpu_map_batch { /* a batch of rule 9 */
  uint32_t first_query, n_queries; /* consecutive query records */
  uint64_t n_anchors, n_query_bases;
  uint64_t n_groups, n_chains, n_pairs;
  uint64_t bytes_bound; /* msgpu_map_batch_bytes of this batch */
  uint64_t bytes_peak;  /* the most bytes the batch held at once */
} msgpu_map_batch;
/* The whole stage.  With ava, queries_path is NULL or the targets' path.  flags must be 0; budget_bytes bounds the bytes of a
 * batch, 0 = the free device memory (rule 9).  Synchronous; the PAF is kept in the result. */
int         msgpu_map_run(msgpu_mapctx *ctx, const msgpu_map_params *params, const char *targets_path, const char *queries_path,
                          uint32_t flags, uint64_t budget_bytes, msgpu_map_result **out);
/* A mapper index that outlives a run: the target file in one of the context's two stores, the
 * per-record offsets and lengths, the target sketch and the index of rule 3 -- everything of a run that depends on the
 * targets, k and w alone.  Of params only k and w matter to msgpu_map_index_create.  The occurrence cap is applied at
 * look-up, so max_occ, like every other parameter, may differ from run to run on one index; a run whose k or w differs
 * from the index's is MSGPU_E_ARG naming both.  With ava, queries_path is NULL and the index's own store and sketch are the
 * query side; otherwise the queries go into the context's other store, so exact mode works on an index, and the store the
 * targets lie in does not matter to any result.  A context holds one index at a time: a second create before the free is
 * MSGPU_E_STATE, an index of another context MSGPU_E_ARG.  A run reads the index and never writes into it: after any
 * error of a run the index is as good as before.  Free the index before its context is destroyed (msgpu_map_destroy frees
 * an index that is still held; it must not be freed again).
 * Stats: n_records[0], n_bases[0], n_minimizers[0], n_keys and n_index_entries of a run come from the index; load_ms,
 * sketch_ms, sort_ms and table_ms of a run on an index cover the query side only (table_ms: rule 3's count of the capped
 * keys at the run's max_occ); the index reports the times of its own build; msgpu_map_run is create, run, free and adds
 * the two, so its stats read as before. */
typedef struct msgpu_map_index msgpu_map_index;
typedef struct msgpu_map_istats {
  uint64_t n_records, n_bases, n_minimizers, n_keys, n_index_entries;
  int32_t  k, w;
  float    load_ms;                       /* host wall: the file into its store */
  float    sketch_ms, sort_ms, table_ms;  /* device, by events */
  float    wall_ms;
  uint32_t reserved;
} msgpu_map_istats;
int         msgpu_map_index_create(msgpu_mapctx *ctx, const msgpu_map_params *params, const char *targets_path,
                                   msgpu_map_index **out);
void        msgpu_map_index_free(msgpu_map_index *index);
int         msgpu_map_index_stats(const msgpu_map_index *index, msgpu_map_istats *out);
int         msgpu_map_run_index(msgpu_mapctx *ctx, const msgpu_map_params *params, const msgpu_map_index *index,
                                const char *queries_path, uint32_t flags, uint64_t budget_bytes, msgpu_map_result **out);
int         msgpu_map_result_stats(const msgpu_map_result *r, msgpu_map_stats *out);
int         msgpu_map_result_chains(const msgpu_map_result *r, const msgpu_map_chain **chains, uint64_t *n);
int         msgpu_map_result_batches(const msgpu_map_result *r, const msgpu_map_batch **batches, uint64_t *n); /* in order */
uint64_t    msgpu_map_result_budget(const msgpu_map_result *r); /* the budget of a batch in bytes: budget_bytes, or what 0 stood for */
const char *msgpu_map_result_text(const msgpu_map_result *r, uint64_t *len);
/* cigar mode (rule 10).  The run tables: the runs of chain i, in output order, are ops[off[i] .. off[i + 1]) (off has n + 1
 * entries), each len << 4 | op with the BAM codes 1 = I, 2 = D, 7 = '=', 8 = X.  Without cigar *n = 0 (and off[0] = 0). */
int         msgpu_map_result_cigars(const msgpu_map_result *r, const uint32_t **ops, const uint64_t **off, uint64_t *n);
typedef struct msgpu_map_astats { /* cigar mode: the segment pairs of rule 10, summed over the batches */
  uint64_t n_pairs_d0, n_pairs_lds, n_pairs_slab, n_pairs_capped; /* no edit; table in LDS; table in the slab; beyond the band */
  uint64_t max_d;                                                 /* the largest distance within the band */
  uint64_t x_columns, i_columns, d_columns;                       /* of the scripts (capped segments not counted) */
  uint64_t script_words, n_runs;                                  /* words of all scripts; runs of all chains */
  uint64_t n_inconsistent; /* pairs whose table contradicted their distance: 0, or the kernels are wrong and the scripts too */
  uint32_t slots, lds_max_d;                                      /* of the slab; the largest d of the LDS class */
  float    align_ms;                                              /* device, by events: offsets, scripts, figures */
  float    cigar_host_ms;                                         /* host: the runs of all chains (wall, summed over the ranges) */
} msgpu_map_astats;
int         msgpu_map_result_align_stats(const msgpu_map_result *r, msgpu_map_astats *out);
/* Rule 11.  msgpu_map_set_extension sets extend on the context for every later msgpu_map_run / msgpu_map_run_index, until it
 * is set again; 0 switches it off.  A value above MSGPU_MAP_EXTEND_MAX is MSGPU_E_ARG, the previous value stays and
 * msgpu_map_last_error names the value.  msgpu_map_batch_bytes_ext is msgpu_map_batch_bytes for a run with that extend (equal
 * to it for extend = 0): what rule 9's cut and bytes_bound use.  msgpu_map_result_ext_stats gives zeros when the feature was
 * off.  msgpu_map_result_ext_ends: the end cells, two per chain in output order, entry 2 i the left end of chain i and
 * 2 i + 1 the right one (*n = 0 when the feature was off). */
#define MSGPU_MAP_EXTEND_MAX 65535u
#define MSGPU_MAP_EXTEND_PENALTY 8
typedef struct msgpu_ext_end { /* the end cell of rule 11.3 */
  uint32_t e;     /* its row: the script has e + 1 words */
  int32_t  k;     /* its diagonal */
  uint32_t x, y;  /* the bytes of A and of B that the extension consumes */
  int32_t  score; /* x + y - P * e */
  uint32_t rows;  /* the rows the end is charged with (rule 11.3) */
} msgpu_ext_end;
typedef struct msgpu_map_xstats { /* rule 11, summed over the batches */
  uint32_t extend, reserved;
  uint64_t n_ends, n_ends_extended, n_ends_at_sequence_end; /* two per chain; x* + y* > 0; the target or the query ends there */
  uint64_t t_bases, q_bases;                                /* sums of x* and of y* */
  uint64_t x_columns, i_columns, d_columns;                 /* of the ends' scripts */
  uint64_t max_e, rows;                                     /* the largest e*; the sum of the ends' rows */
  uint64_t n_inconsistent; /* ends whose table contradicted itself on the walk: 0, or the kernel is wrong */
  float    extend_ms;      /* device, by events: descriptors and extension */
} msgpu_map_xstats;
int         msgpu_map_set_extension(msgpu_mapctx *ctx, uint32_t extend);
int         msgpu_map_result_ext_stats(const msgpu_map_result *r, msgpu_map_xstats *out);
int         msgpu_map_result_ext_ends(const msgpu_map_result *r, const msgpu_ext_end **ends, uint64_t *n);
uint64_t    msgpu_map_batch_bytes_ext(const msgpu_map_params *params, uint32_t extend, uint64_t n_anchors, uint64_t n_query_bases);
/* Rule 12.  msgpu_map_set_ranking switches it on (on != 0) or off for every later msgpu_map_run / msgpu_map_run_index, until it
 * is set again.  msgpu_map_result_ranks: entry i belongs to line i; *n = 0 when ranking was off.  msgpu_map_result_rank_stats
 * gives zeros when it was off.  msgpu_map_rank_tables is the table-level entry (as msgpu_extend_ends is rule 11's): rule 12 on
 * n chains of the host in output order, copied to the device; parent is relative to that table; of a chain only query,
 * n_anchors, score, q_start and q_end are read.  query must not decrease and q_start <= q_end, else MSGPU_E_ARG naming the
 * first bad chain: a device pass, complete before any ranking kernel runs.  n = 0 is fine.  msgpu_map_rank_tables_stats: the
 * counts of the context's last msgpu_map_rank_tables (zeros after an error).
 * MSGPU_MAP_RANK_LDS: the primaries of a segment of more than 64 chains that the list kernel keeps in LDS; the ones beyond lie
 * in the batch arena, and the segment is counted in n_segments_spilled. */
#define MSGPU_MAP_RANK_LDS 512u
typedef struct msgpu_map_rank { /* in output order: entry i belongs to chain i */
  uint32_t parent;      /* the chain's primary; its own index for a primary */
  int32_t  sub;         /* rule 12.3 */
  uint32_t n_secondary; /* rule 12.3 */
  uint32_t mapq;        /* rule 12.4 */
} msgpu_map_rank;
typedef struct msgpu_map_rstats { /* rule 12, summed over the batches; a segment is the chains of one query record */
  uint32_t ranking, lds_primaries;                                   /* the switch; MSGPU_MAP_RANK_LDS */
  uint64_t n_segments, n_primaries, n_secondaries, n_mapq0;          /* n_mapq0: chains with mapq 0, the secondaries among them */
  uint64_t largest_segment;
  uint64_t n_segments_single, n_segments_wave, n_segments_list;      /* one chain; 2..64 (a wavefront); more (the list kernel) */
  uint64_t n_segments_spilled;                                       /* list segments with more than lds_primaries primaries */
  float    rank_ms, reserved2;                                       /* device, by events */
} msgpu_map_rstats;
int         msgpu_map_set_ranking(msgpu_mapctx *ctx, int on);
int         msgpu_map_result_ranks(const msgpu_map_result *r, const msgpu_map_rank **ranks, uint64_t *n);
int         msgpu_map_result_rank_stats(const msgpu_map_result *r, msgpu_map_rstats *out);
uint64_t    msgpu_map_batch_bytes_rank(const msgpu_map_params *params, uint32_t extend, uint32_t ranking, uint64_t n_anchors,
                                       uint64_t n_query_bases);
int         msgpu_map_rank_tables(msgpu_mapctx *ctx, const msgpu_map_chain *chains, uint64_t n, msgpu_map_rank *ranks_out);
int         msgpu_map_rank_tables_stats(const msgpu_mapctx *ctx, msgpu_map_rstats *out);
/* Rule 13.  msgpu_map_set_mates switches it on (on != 0) or off and sets max_insert for every later msgpu_map_run /
 * msgpu_map_run_index, until it is set again; a max_insert outside 1..2^31 - 1 is MSGPU_E_ARG, the previous values stay and
 * msgpu_map_last_error names the value.  msgpu_map_result_mates: entry i belongs to line i; *n = 0 when mates was off.
 * msgpu_map_result_mate_stats gives zeros when it was off.  msgpu_map_mate_tables is the table-level entry (as
 * msgpu_map_rank_tables is rule 12's): rule 13 on n chains of the host in output order, copied to the device; mate is relative
 * to that table; of a chain only query, target, strand, score, t_start and t_end are read.  query must not decrease,
 * strand <= 1 and t_start <= t_end, else MSGPU_E_ARG "chain <i>: order", "chain <i>: strand" or "chain <i>: range", naming the
 * smallest bad chain and the first violated of the three: a device pass, complete before any mates kernel runs.  n = 0 is
 * fine.  The table knows the pairs with a chain only: its n_pairs counts those and n_unmapped is 0.
 * msgpu_map_mate_tables_stats: the counts of the context's last msgpu_map_mate_tables (zeros after an error).
 * MSGPU_MAP_MATES_ANCHOR_BYTES, MSGPU_MAP_MATES_FIXED_BYTES: what msgpu_map_batch_bytes_mates adds per anchor and once. */
#define MSGPU_MAP_MATES_ANCHOR_BYTES 60u
#define MSGPU_MAP_MATES_FIXED_BYTES (12u * 256u)
#define MSGPU_MAP_MAX_INSERT_DEFAULT 1000u
typedef struct msgpu_map_mate { /* in output order: entry i belongs to chain i */
  uint32_t mate;   /* the selected mate's chain; 0xffffffff for a chain that is not selected */
  uint32_t tlen;   /* rule 13.1's tl of the selected combination */
  uint32_t cls;    /* 1: selected (a proper pair's chain); 0: not */
  uint32_t n_best; /* rule 13.2 */
} msgpu_map_mate;
typedef struct msgpu_map_mstats { /* rule 13, summed over the batches */
  uint32_t mates, max_insert;                                         /* the switch; the parameter (0 when off) */
  uint64_t n_pairs, n_proper, n_ambiguous, n_discordant, n_single, n_unmapped;
  uint64_t n_pairs_settled, n_pairs_lanes16, n_pairs_lanes64, n_pairs_list; /* by kernel: the classifier (a mate without a chain, or
                                                                         one chain each); at most 16 chains; at most 64; more */
  uint64_t largest_pair;                                              /* in chains */
  uint64_t tlen_sum, tlen_min, tlen_max;                              /* over the proper pairs; 0 without one */
  float    mate_ms, reserved2;                                        /* device, by events */
} msgpu_map_mstats;
int         msgpu_map_set_mates(msgpu_mapctx *ctx, int on, uint32_t max_insert);
int         msgpu_map_result_mates(const msgpu_map_result *r, const msgpu_map_mate **mates, uint64_t *n);
int         msgpu_map_result_mate_stats(const msgpu_map_result *r, msgpu_map_mstats *out);
uint64_t    msgpu_map_batch_bytes_mates(const msgpu_map_params *params, uint32_t extend, uint32_t ranking, uint32_t mates,
                                        uint64_t n_anchors, uint64_t n_query_bases);
int         msgpu_map_mate_tables(msgpu_mapctx *ctx, const msgpu_map_chain *chains, uint64_t n, uint32_t max_insert,
                                  msgpu_map_mate *rows_out);
int         msgpu_map_mate_tables_stats(const msgpu_mapctx *ctx, msgpu_map_mstats *out);
void        msgpu_map_result_free(msgpu_map_result *r);

/* ---- pileup consensus: polishing a draft from the mapper's run tables ------------------------------
 * Every chain of reads against a draft, as the mapper's cigar mode gives it (a chain table and the run tables of
 * msgpu_map_result_cigars, the reads as queries and the draft as targets), votes on the draft's bases; the polished FASTA is
 * written.  The reference tree has no polisher: the stage is defined by the rules below, in integers only, and is checked
 * without tolerance against their restatement in plain Python (tests/pl_oracle.py).  Both files go through
 * msgpu_seq_parse_upload, as the mapper's do.  Parameters: min_depth (>= 1, default 3), min_identity (a percentage, 0..100,
 * default 0).
 *  1. tables.  off[0] = 0 and off never decreases (checked first: nothing else can be read without it).  Then, per chain i
 *     with runs ops[off[i] .. off[i + 1]): (a) its query record is not smaller than chain i - 1's; (b) strand is 0 or 1;
 *     (c) the query record and (d) the target record are in range; (e) t_start < t_end <= tlen; (f) q_start <= q_end <= qlen;
 *     (g) every run has len >= 1 and an op in {1 = I, 2 = D, 7 = '=', 8 = X}; (h) the runs consume exactly t_end - t_start
 *     target bases ('=', X, D) and (i) q_end - q_start query bases ('=', X, I); a run that breaks (g) consumes nothing.  The
 *     violation reported is that of the smallest chain index, and of that chain the first in the order (a) .. (i):
 *     MSGPU_E_ARG, the text "chain <i>: <what>".  The check is a device pass that publishes the smallest bad chain through the
 *     scalar block, and it is complete before any kernel walks a run: a bad table ends in an error, never in a fault.
 *     In ranked form (msgpu_pl_run_ranked) a check (j) is added and reported last: the rank row's parent is in range and names
 *     a chain of the same query record that is its own parent, and mapq <= 60; otherwise "chain <i>: rank".
 *     In mates form (msgpu_pl_run_mates) a check (k) is added and reported last: cls <= 1 on every row, and for a row with
 *     cls == 1 the mate is in range, the mate's row has cls == 1 and names this chain, the mate's query record is this
 *     one's ^ 1, and n_best >= 1; otherwise "chain <i>: mates".
 *  2. voters.  A chain is eligible iff matches * 100 >= min_identity * block.  Per query record the voter is the eligible
 *     chain with the greatest score, then the greatest block, then the first in table order.  Every other chain is ignored
 *     and counted.  Ranked form (msgpu_pl_run_ranked, with the mapper's rule 12 rows): a chain votes iff it is eligible,
 *     primary (parent == its own index) and mapq >= min_mapq.  So a read may have several voters (a split alignment votes
 *     with every part), a secondary never votes, and a read placed equally on two repeat copies (mapq 0) votes only at
 *     min_mapq = 0.  Everything behind the voters' spans is the same in both forms.  Mates form (msgpu_pl_run_mates, with
 *     the mapper's rule 13 rows): a chain votes iff it is eligible, selected (cls == 1) and n_best == 1.  So a pair placed
 *     equally well twice does not vote, an unselected chain never votes, and a read inside a repeat copy votes on the copy
 *     that its mate names.  Everything behind the voters' spans is the same code in all three forms.
 *  3. oriented query.  Column j of a chain reads byte q_start + j_q of the query for strand 0 (j_q: the query bases that the
 *     columns in front of j consume); for strand 1 the oriented query is MSGPU_COPY_REVCOMP's of the whole record (reversed,
 *     A <-> T and C <-> G in upper case, every other byte as it is), and the chain starts at qlen - q_end in it.  The byte is
 *     then folded to upper case; A, C, G and T vote for themselves, any other byte votes "other".
 *  4. pile-up.  Per draft base six 32-bit counters: A, C, G, T, del, other.  An '=' or X column of a voter adds the class of
 *     its query byte at its target position, a D column adds del; depth(p) is the sum of the six.  An I run of length L of a
 *     voter that lies between target positions p - 1 and p is one insertion event at slot p; it is usable iff L <= 32 and
 *     all its bytes are A, C, G or T, and is then keyed (slot, L, the letters packed at 2 bits, the first in the highest
 *     bits); an unusable event is counted and ignored, and so is an I run that is the first or the last run of its chain.
 *  5. call, per position p.  depth(p) < min_depth, or A = C = G = T = del = 0: the draft's byte, verbatim.  Else the winner
 *     is the greatest of A, C, G, T, del; on a tie the draft's own folded base if it is among the tied, else the first of
 *     A, C, G, T, del.  The winner is the draft's folded base: the draft's byte, verbatim (case is kept: a polish that
 *     changes nothing is the identity on bytes); del: nothing; else the winner's upper-case letter.
 *  6. insertions, per slot p with 0 < p < tlen of a record: the usable events are grouped by (L, letters); the candidate is
 *     the group with the greatest count, then the smaller L, then the smaller packed letters; with
 *     m = min(depth(p - 1), depth(p)) it is applied iff m >= min_depth and 2 * count > m, and its letters are emitted in
 *     front of position p's call.  (Usable events at other slots are counted and never applied.)
 *  7. output.  The records in the draft's order: '>' + the cleaned name + '\n', then the bases wrapped by msgpu_fasta_format
 *     (60 columns); a record that comes out without bases is the header and an empty line, as msgpu_fasta_format writes a
 *     length of 0.  On any error nothing is written.
 *  8. limits, each an error and never a fault: the file limits are the mapper's (a record below 2^31 bases, a file below
 *     2^38); fewer than 2^31 chains and runs, fewer than 2^40 columns of voters, a polished record below 2^32 bases.  Device
 *     memory: the six counters per draft base with the slot's winner, the call, the output length and its scan (45 bytes per
 *     base), 40 bytes per run, the insertion events with their sort buffers (60 bytes per event) and the output (raw bases
 *     and text) must fit beside the two stores, else MSGPU_E_NOMEM naming the sizes.  Batching over reads is out of scope. */
typedef struct msgpu_plctx msgpu_plctx; /* a device context of the stage */
typedef struct msgpu_pl_result msgpu_pl_result;
typedef struct msgpu_pl_params {
  int32_t min_depth, min_identity;
} msgpu_pl_params;
typedef struct msgpu_pl_stats {
  uint64_t n_records, n_bases, n_reads, n_read_bases;  /* the draft; the read file */
  uint64_t n_chains, n_runs, n_voters, n_ignored;      /* rule 2 */
  uint64_t cols_eq, cols_x, cols_d, cols_i;            /* the voters' columns by op (I: every I run, whatever becomes of it) */
  uint64_t pos_verbatim, pos_unchanged, pos_substituted, pos_deleted; /* rule 5: no call made; the draft's base won; ... */
  uint64_t ins_usable, ins_unusable, ins_at_ends;      /* rule 4: the insertion events */
  uint64_t ins_applied, bases_inserted;                /* rule 6 */
  uint64_t max_depth;
  uint64_t n_lost_publications, bytes_out, bytes_peak; /* bytes_peak: the most device bytes the run held beside the stores */
  msgpu_pl_params params;
  float load_ms;                                       /* host wall: both files into their stores */
  float validate_ms, offsets_ms, voters_ms, pileup_ms, insertions_ms, call_ms, output_ms, format_ms, copy_ms; /* device, by events */
  float wall_ms;
  uint32_t reserved;
} msgpu_pl_stats;
typedef struct msgpu_pl_record { /* per draft record */
  uint64_t len_in, len_out, n_substituted, n_deleted, n_inserted; /* n_inserted: insertions applied, not their bases */
  uint64_t depth_x100;                                            /* floor(100 * sum of depth(p) / len_in); 0 for len_in = 0 */
} msgpu_pl_record;
void        msgpu_pl_default_params(msgpu_pl_params *p);
int         msgpu_pl_create(int device, msgpu_plctx **out); /* MSGPU_E_NODEVICE without a GPU */
void        msgpu_pl_destroy(msgpu_plctx *ctx);
const char *msgpu_pl_last_error(const msgpu_plctx *ctx);
/* The whole stage.  chains: n_chains entries; off: n_chains + 1 entries; ops: off[n_chains] entries (host tables, copied).
 * flags is 0 or MSGPU_PL_VCF (below; here and in the two forms that follow).  Synchronous; the FASTA is kept in the result. */
int         msgpu_pl_run(msgpu_plctx *ctx, const msgpu_pl_params *params, const char *draft_path, const char *reads_path,
                         const msgpu_map_chain *chains, uint64_t n_chains, const uint32_t *ops, const uint64_t *off, uint32_t flags,
                         msgpu_pl_result **out);
/* The stage with rule 2 in ranked form: ranks holds n_chains rows of the mapper's rule 12 (msgpu_map_result_ranks or
 * msgpu_map_rank_tables; parent indexes this chain table), checked by rule 1 (j).  msgpu_pl_run is untouched by it. */
int         msgpu_pl_run_ranked(msgpu_plctx *ctx, const msgpu_pl_params *params, const char *draft_path, const char *reads_path,
                                const msgpu_map_chain *chains, uint64_t n_chains, const uint32_t *ops, const uint64_t *off,
                                const msgpu_map_rank *ranks, uint32_t min_mapq, uint32_t flags, msgpu_pl_result **out);
/* The stage with rule 2 in mates form: mates holds n_chains rows of the mapper's rule 13 (msgpu_map_result_mates or
 * msgpu_map_mate_tables; mate indexes this chain table), checked by rule 1 (k).  msgpu_pl_run and msgpu_pl_run_ranked are
 * untouched by it. */
int         msgpu_pl_run_mates(msgpu_plctx *ctx, const msgpu_pl_params *params, const char *draft_path, const char *reads_path,
                               const msgpu_map_chain *chains, uint64_t n_chains, const uint32_t *ops, const uint64_t *off,
                               const msgpu_map_mate *mates, uint32_t flags, msgpu_pl_result **out);
const char *msgpu_pl_result_text(const msgpu_pl_result *r, uint64_t *len);
int         msgpu_pl_result_stats(const msgpu_pl_result *r, msgpu_pl_stats *out);
int         msgpu_pl_result_records(const msgpu_pl_result *r, const msgpu_pl_record **records, uint64_t *n);
void        msgpu_pl_result_free(msgpu_pl_result *r);

/* What the polisher changed, as VCF 4.2 formatted on the device (msgpu_vcf.hip).  On request only: bit
 * MSGPU_PL_VCF of the `flags` of msgpu_pl_run, msgpu_pl_run_ranked and msgpu_pl_run_mates (any other bit stays MSGPU_E_ARG).
 * Without the bit no kernel of it is launched and no byte allocated; with it the FASTA, the record table and every field of
 * msgpu_pl_stats but bytes_peak, wall_ms and the times are those of the run without it.  The rules, per draft record of tlen
 * bases; e(p): rule 5 substituted or deleted position p; ins(p): the letters rule 6 applies at slot p (empty for p = 0 and
 * p = tlen):
 *  V1. blocks.  A block is a maximal run [a, b) of positions with e(p); it owns the applied insertions at slots a .. b, both
 *      ends included.  An applied insertion at a slot p with neither e(p - 1) nor e(p) is a block of its own with a = b = p.
 *      Every position heads at most one block, and blocks never touch: an unchanged position lies between two of them.
 *  V2. alleles.  REF0 = the draft's bytes of [a, b), folded to upper case, any byte outside ACGT written N.  ALT0 =
 *      ins(a) call(a) ins(a + 1) call(a + 1) ... call(b - 1) ins(b), for a = b ins(a) alone: the bytes the polisher emits for
 *      the block, always upper-case ACGT.
 *  V3. anchoring.  Both non-empty: POS = a + 1, REF = REF0, ALT = ALT0 (MSGPU_VCF_ANCHOR_NONE).  One of them empty and a > 0:
 *      the draft's byte at a - 1 (unchanged by maximality; folded, non-ACGT as N) is put in front of both, POS = a
 *      (MSGPU_VCF_ANCHOR_LEFT).  One empty, a = 0 and b < tlen: the draft's byte at b is put behind both, POS = 1
 *      (MSGPU_VCF_ANCHOR_RIGHT).  a = 0 and b = tlen, the whole record deleted: POS = 1, REF = the folded first base, ALT =
 *      <DEL>, and INFO gains END=<tlen> in front of DP (MSGPU_VCF_ANCHOR_WHOLE).  Indels inside repeats are not left-aligned:
 *      positions are where the alignment put them (out of scope).
 *  V4. INFO, integers only.  DP = the minimum of depth(p) over [a, b), for a = b min(depth(a - 1), depth(a)).  AO = the minimum
 *      over the block's edits of their support: the winning counter at an edited position, the applied group's count at an
 *      applied slot.  TYPE = ins if REF0 is empty; del if ALT0 is empty; snp or mnp if |REF0| = |ALT0| (1, or more) and the
 *      block holds neither a deletion nor an insertion; complex otherwise.
 *  V5. line.  <name> TAB <POS> TAB . TAB <REF> TAB <ALT> TAB . TAB PASS TAB [END=n;]DP=d;AO=a;TYPE=t LF.  Lines come in
 *      draft-record order, then by a.
 *  V6. header, written on the host as the FASTA headers are: ##fileformat=VCFv4.2, ##source=muchsalsa_amd.polish, one
 *      ##contig=<ID=name,length=tlen> per draft record in order, ##INFO lines for DP, AO, TYPE and END, ##ALT=<ID=DEL,...>, and
 *      the #CHROM ... INFO line without sample columns.  A draft without variants is the header alone.
 *  V7. names, checked only when VCF is asked for: a draft record is refused with MSGPU_E_ARG naming the record if its cleaned
 *      name is empty, longer than 254 bytes, holds a byte outside 0x21..0x7e or one of , < >, begins with * or =, or repeats
 *      an earlier record's name.  Nothing is written in that case, and the context goes on.
 *  V8. rounds.  A VCF's coordinates are those of the draft of its own round: muchsalsa_amd.polish refuses VCF together with
 *      more than one round (TypeError; from the command usage and exit status 2).
 *  V9. limits, each an error and never a fault: fewer than 2^31 blocks; decimal widths up to the existing limits of positions
 *      and depths; the extra device memory (12 bytes per draft base: the flag word and its scan; per block the row, the size
 *      and its scan and the two class lists, 72 bytes; the text) is compared with what is free where the number of blocks and
 *      the text size are known, else MSGPU_E_NOMEM naming the sizes.  The text's size by the scan is checked against a bound
 *      from the stage's own counts and against the lines by class; a mismatch is MSGPU_E_STATE. */
#define MSGPU_PL_VCF 1u           /* flags: write the VCF too */
#define MSGPU_VCF_SHORT_BYTES 512u /* a line of at most this many bytes is written by one wavefront, a longer one by 8 workgroups */
#define MSGPU_VCF_LINE_FIXED 96u  /* the part of a line's text bound beside its name and its alleles */
enum { MSGPU_VCF_SNP = 0, MSGPU_VCF_MNP = 1, MSGPU_VCF_INS = 2, MSGPU_VCF_DEL = 3, MSGPU_VCF_COMPLEX = 4 };
enum { MSGPU_VCF_ANCHOR_NONE = 0, MSGPU_VCF_ANCHOR_LEFT = 1, MSGPU_VCF_ANCHOR_RIGHT = 2, MSGPU_VCF_ANCHOR_WHOLE = 3 };
typedef struct msgpu_pl_variant { /* per block, in the order of the lines; 48 bytes */
  uint32_t record, a, ref_len, alt_len; /* the draft record; [a, a + ref_len) = REF0; |ALT0| */
  uint32_t dp, ao, type, anchor;        /* V4; MSGPU_VCF_*; MSGPU_VCF_ANCHOR_* */
  uint64_t offset, length;              /* the line in the text of msgpu_pl_result_vcf */
} msgpu_pl_variant;
typedef struct msgpu_pl_vcf_stats {
  uint64_t n_variants, n_snp, n_mnp, n_ins, n_del, n_complex, n_whole_deleted;
  uint64_t n_short, n_long;          /* the lines by class (MSGPU_VCF_SHORT_BYTES) */
  uint64_t ref_bases, alt_bases;     /* the sums of |REF0| and of |ALT0| */
  uint64_t header_bytes, text_bytes; /* text_bytes: the whole text, the header included */
  uint64_t bytes_peak;               /* the most device bytes the run held beside the stores, VCF included */
  float    vcf_ms;                   /* device, by events: everything of the VCF */
  uint32_t reserved;
} msgpu_pl_vcf_stats;
/* The text (NULL and 0 when it was not asked for), the rows and the counts (zeroed when it was not asked for). */
const char *msgpu_pl_result_vcf(const msgpu_pl_result *r, uint64_t *len);
int         msgpu_pl_result_variants(const msgpu_pl_result *r, const msgpu_pl_variant **rows, uint64_t *n);
int         msgpu_pl_result_vcf_stats(const msgpu_pl_result *r, msgpu_pl_vcf_stats *out);

/* ---- SAM output: the mapper's tables as SAM 1.6 text, formatted on the device ---------------------
 * The chain table of a mapper run with its run tables (msgpu_map_result_cigars), rank rows (rule 12) and, for pairs, mate rows
 * (rule 13) becomes the text that samtools, IGV and variant callers read.  The stage is additive: nothing else changes by
 * it.  It loads both files itself through msgpu_seq_parse_upload, as the polisher does.  Parameters: eqx (0 / 1, default 1),
 * md (0 / 1, default 0), unmapped (0 / 1, default 1).  The stage is defined by the rules below, in integers only, and checked,
 * without tolerance, against the tests' restatement in plain Python (tests/sam_oracle.py), not against another tool:
 *  S1. inputs and checks.  Both files through msgpu_seq_parse_upload; the chain table in output order; the run tables (runs
 *      of chain i: ops[off[i] .. off[i + 1]), each len << 4 | op); the rank rows (required); optionally the mate rows.  The
 *      checks are complete on the device before any formatting kernel runs; a failure is MSGPU_E_ARG "chain <i>: <what>" for
 *      the smallest bad chain and, of that chain, the first violated check in this order: (a) off[0] = 0, the offsets do not
 *      decrease (and none exceeds off[n_chains], the size of the run table); (b) query does not decrease; (c) strand <= 1;
 *      (d) the query record and the target record are in range; (e) t_start <= t_end <= tlen; (f) q_start <= q_end <= qlen;
 *      (g) every op is one of 1 (I), 2 (D), 7 (=), 8 (X) with length > 0 (a run that breaks this consumes nothing); (h) the
 *      runs consume exactly t_end - t_start target bases and (i) q_end - q_start query bases; (j) parent is in range, lies in
 *      the same query record and names a chain that is its own parent; (k) with mates, for a chain with cls = 1: mate is in
 *      range, lies in the partner record (query ^ 1) and its row has cls = 1 and points back.  With mates an odd number of query
 *      records is MSGPU_E_ARG naming the count.  Host checks, each MSGPU_E_ARG naming the record: two target records with the
 *      same name (the loader keeps the first record of a name and drops the later ones, so a file cannot bring this about:
 *      the records, and the chain table's indices, are those the loader keeps, and the check guards the header); a name
 *      longer than 254 bytes; an empty name (both files).
 *  S2. header.  "@HD\tVN:1.6\tSO:unsorted\tGO:query", one "@SQ\tSN:<name>\tLN:<length>" per target record in file order,
 *      "@PG\tID:muchsalsa_amd\tPN:muchsalsa_amd"; nothing else (no version, no command line): the text is a function of the
 *      inputs alone.
 *  S3. lines and their order.  One line per chain, in the chain table's order.  With unmapped = 1 a query record without a
 *      chain gets one unmapped line in its place in query record order: every read appears, and a pair's lines are adjacent.
 *  S4. roles within a query record.  The representative is the rank-primary chain (parent == own index) with the greatest
 *      score, the smallest index on a tie.  The other primaries are supplementary (0x800), the rank-secondaries secondary
 *      (0x100).
 *  S5. clips and CIGAR.  With oq the oriented query: left clip = q_start on strand 0, qlen - q_end on strand 1; right clip =
 *      the other remainder.  The CIGAR is the left clip, the runs, the right clip; zero-length clips are left out; a CIGAR
 *      without any run or clip is '*'.  The representative clips with S, supplementary and secondary lines with H.  With
 *      eqx = 1 the runs are written as they are (=, X, I, D); with eqx = 0 every maximal stretch of neighbouring = and X runs
 *      becomes one M run.
 *  S6. SEQ.  A byte is folded to upper case; A, C, G, T stay (on strand 1 they are complemented and the read reversed); every
 *      other byte becomes N.  Representative: the whole oriented read.  Supplementary: oq's aligned part only.  Secondary: '*'.
 *      Unmapped: the read as the file holds it, folded the same way.  A SEQ without bases is '*'.  QUAL is always '*'.  (The
 *      = / X letters are rule 10's, on the bytes as the stores hold them: on lower-case or non-ACGT input they can disagree
 *      with a comparison of SEQ against the reference; on upper-case ACGT input they cannot.)
 *  S7. columns of a chain line.  QNAME: the query name; with mates a trailing "/1" or "/2" is removed when the name is longer
 *      than two bytes.  FLAG: S8.  RNAME: the target name.  POS: t_start + 1.  MAPQ: the rank row's mapq.  CIGAR: S5.  RNEXT,
 *      PNEXT, TLEN: S8.  SEQ, QUAL: S6.  Then the tags, in this order: NM:i:<nm>, AS:i:<score>, cm:i:<n_anchors>, s2:i:<sub>
 *      (representative and supplementary lines only), tp:A:P (primaries) or tp:A:S (secondaries), nb:i:<n_best> (lines with
 *      cls = 1 only), MD:Z:<md> (with md = 1).
 *  S8. FLAG and the mate columns.  0x10 iff strand = 1; 0x100 and 0x800 by S4.  Without mates: RNEXT '*', PNEXT 0, TLEN 0.
 *      With mates: 0x1 on every line; 0x40 on the lines of record 2p, 0x80 on those of record 2p + 1; 0x2 iff cls = 1.  The
 *      mate line of a chain is `mate` if cls = 1, else the representative of the partner record, else none.  If it exists:
 *      0x20 iff it is on strand 1; RNEXT is '=' on the same target, else its target's name; PNEXT is its POS; on the same
 *      target TLEN's magnitude is max(t_end) - min(t_start) over the two, positive on the line with the smaller t_start and
 *      negative on the other, on equal t_start the line of record 2p is the positive one (for a proper pair this is +- rule
 *      13's tl); on different targets TLEN is 0.  If no mate line exists: 0x8, RNEXT '=', PNEXT = own POS, TLEN 0.
 *  S9. unmapped lines.  FLAG 0x4, plus 0x1 and 0x40 / 0x80 with mates.  With a mate line (paired only: the representative of
 *      the partner record): 0x20 iff it is reverse; RNAME and POS are the mate line's; RNEXT '='; PNEXT is the mate line's
 *      POS; TLEN 0.  Without: 0x8 too when paired; RNAME '*', POS 0, RNEXT '*', PNEXT 0, TLEN 0.  In both cases MAPQ 0,
 *      CIGAR '*', no tags.
 * S10. MD (with md = 1).  Walk the runs with the target bytes folded as in S6 (no complement).  = columns add to a running
 *      count; an X column writes the count, the target base, and resets the count; a D run writes the count, '^', the target
 *      bases, and resets the count; I runs do nothing (they do not split a count); the final count is written.  So the string
 *      begins and ends with a number; neighbouring mismatches, and a mismatch next to a deletion, are separated by 0.
 * S11. batches and limits.  Resident for a run: the two stores, the names, the chain, rank and mate rows with every chain's
 *      FLAG and mate line, the run tables with their scans.  Per batch of consecutive query records (whole pairs with mates):
 *      the line table, the per-line sizes and their 64-bit scan, the class lists, the text.  A line's text bound is
 *      1024 + qlen + 11 * (runs + 2), with md = 1 plus 2 * (t_end - t_start) + 11 * (runs + 1); an unmapped line's is
 *      1024 + qlen.  msgpu_sam_batch_bytes(params, lines, text bound) bounds the device bytes of a batch; the cut is the
 *      mapper's greedy cut (rule 9) on msgpu_sam_batch_bytes <= budget with fewer than 2^31 lines per batch; budget_bytes = 0
 *      stands for the free device memory once the resident part is allocated (an eighth less, again and again, while the
 *      device cannot give the largest batch's bytes as one block).  The batches' texts one behind the other, behind the header,
 *      are the file.  A record (with mates: a pair) that exceeds the budget alone is MSGPU_E_NOMEM naming it.  Fewer than 2^31
 *      chains and runs, fewer than 2^32 lines; the file limits are the mapper's.  Every limit is an error, never a fault.  On
 *      any error there is no result.
 * For instance target t = ACGTACGTACGTACGTACGT, query q = TTCGTGGTAACG, one chain: strand 0, q 2..11, t 5..14, runs
 * 3= 1X 1D 2= 1I 2=, score 40, 3 anchors, primary, mapq 60, with md = 1:
 *   q\t0\tt\t6\t60\t2S3=1X1D2=1I2=1S\t*\t0\t0\tTTCGTGGTAACG\t*\tNM:i:3\tAS:i:40\tcm:i:3\ts2:i:0\ttp:A:P\tMD:Z:3A0^C4
 * and with eqx = 0 the CIGAR is 2S4M1D2M1I2M1S.
 * Out of scope: base qualities (the stores keep none), the SA:Z and MC:Z tags, BAM, coordinate sorting. */
typedef struct msgpu_samctx msgpu_samctx; /* a device context of the stage */
typedef struct msgpu_sam_result msgpu_sam_result;
typedef struct msgpu_sam_params {
  int32_t eqx, md, unmapped, reserved; /* defaults 1, 0, 1, 0 */
} msgpu_sam_params;
#define MSGPU_SAM_UNMAPPED 0xffffffffu  /* msgpu_sam_line.chain of an unmapped line */
#define MSGPU_SAM_LINE_FIXED 1024u      /* S11: the part of a line's text bound that does not depend on the line */
#define MSGPU_SAM_SHORT_BYTES 2048u     /* a line of at most this many bytes is written by one wavefront, a longer one by 8 workgroups */
typedef struct msgpu_sam_line { /* per alignment line, in file order */
  uint32_t chain;    /* MSGPU_SAM_UNMAPPED: an unmapped line */
  uint32_t query, flag, reserved;
  uint64_t offset;   /* of the line's first byte in the text */
} msgpu_sam_line;
typedef struct msgpu_sam_batch { /* a batch of S11, modelled on msgpu_map_batch */
  uint32_t first_query, n_queries; /* consecutive query records */
  uint64_t n_lines, text_bound;
  uint64_t n_short, n_long;        /* lines by class */
  uint64_t text_bytes;
  uint64_t bytes_bound;            /* msgpu_sam_batch_bytes of this batch */
  uint64_t bytes_peak;             /* the most bytes the batch held at once */
} msgpu_sam_batch;
typedef struct msgpu_sam_stats {
  uint64_t n_targets, n_queries, n_chains, n_runs;
  uint64_t n_lines, n_representative, n_supplementary, n_secondary, n_unmapped;
  uint64_t n_short, n_long;                     /* lines by class */
  uint64_t n_batches, budget_bytes;             /* budget_bytes: what a batch had (budget_bytes of the call, or what 0 stood for) */
  uint64_t header_bytes, bytes_out, bytes_peak; /* bytes_peak: the most device bytes held beside the stores, resident part and batch */
  uint64_t n_lost_publications;
  msgpu_sam_params params;
  float load_ms;                                /* host wall: both files into their stores */
  float validate_ms, scan_ms, roles_ms, format_ms, copy_ms; /* device, by events; format_ms: line table, sizes, scan and write */
  float wall_ms;
  uint32_t reserved;
} msgpu_sam_stats;
void        msgpu_sam_default_params(msgpu_sam_params *p);
int         msgpu_sam_create(int device, msgpu_samctx **out); /* MSGPU_E_NODEVICE without a GPU */
void        msgpu_sam_destroy(msgpu_samctx *ctx);
const char *msgpu_sam_last_error(const msgpu_samctx *ctx);
/* S11's bound on the device bytes of a batch.  A host function without a device call. */
uint64_t    msgpu_sam_batch_bytes(const msgpu_sam_params *params, uint64_t n_lines, uint64_t text_bound);
/* The whole stage.  chains, ranks (and mates, or NULL: single-end): n_chains entries; off: n_chains + 1 entries; ops:
 * off[n_chains] entries (host tables, copied).  flags must be 0.  Synchronous; the text is kept in the result. */
int         msgpu_sam_run(msgpu_samctx *ctx, const msgpu_sam_params *params, const char *targets_path, const char *queries_path,
                          const msgpu_map_chain *chains, uint64_t n_chains, const uint32_t *ops, const uint64_t *off,
                          const msgpu_map_rank *ranks, const msgpu_map_mate *mates, uint32_t flags, uint64_t budget_bytes,
                          msgpu_sam_result **out);
const char *msgpu_sam_result_text(const msgpu_sam_result *r, uint64_t *len);
int         msgpu_sam_result_stats(const msgpu_sam_result *r, msgpu_sam_stats *out);
int         msgpu_sam_result_lines(const msgpu_sam_result *r, const msgpu_sam_line **lines, uint64_t *n);
int         msgpu_sam_result_batches(const msgpu_sam_result *r, const msgpu_sam_batch **batches, uint64_t *n); /* in order */
void        msgpu_sam_result_free(msgpu_sam_result *r);

/* ---- between the overlap path and assemblePath (host) -----------------------------
 * graph clean-up (src/main.cpp:194-288, 465-618: contraction targets and roots, ContainElements, deletions,
 * computeBitweight, getMaxSpanTree mst.cpp:34-111, decycle), getConnectedComponents (cc.cpp:33-70) and, per component,
 * getDirectedGraph (dg.cpp:35-121) + linearizeGraph (lg.cpp:41-629) as the assemblePaths job does (main.cpp:620-661).
 * Input: the tables of msgpu_copy_tables / msgpu_copy_reads (copied) and the result of msgpu_find_contraction_edges.
 * Output: one msgpu_path_input per linearised path, ready for msgpu_assembly_add_paths.  Iteration orders the
 * reference leaves to hash containers follow DESIGN.md section 2, "canonical order".  MSGPU_E_LAYOUT = the reference would terminate. */
typedef struct msgpu_graph msgpu_graph;
typedef struct msgpu_graph_stats {
  uint64_t n_vertices_in, n_edges_in;
  uint64_t n_contraction_edges, n_deleted_vertices, n_contain_elements, n_decycled_edges;
  uint64_t n_vertices, n_edges; /* after the clean-up */
  uint64_t n_components, n_paths, n_path_reads;
} msgpu_graph_stats;
/* The four tables are COPIED (read_len / read_first_line always are).  ems = NULL (n_ems ignored): no EdgeMatch table on
 * the host -- the graph stage itself never reads one; the EdgeMatches of the path edges, which assemblePath needs
 * (dg.cpp:99-101), are supplied after msgpu_graph_linearize through msgpu_graph_path_edges + msgpu_get_edgematches +
 * msgpu_graph_set_path_edgematches. */
int  msgpu_graph_create(const msgpu_edge *edges, uint64_t n_edges, const msgpu_edgematch *ems, uint64_t n_ems,
                        const msgpu_order *orders, uint64_t n_orders, const uint32_t *ids, uint64_t n_ids,
                        const int32_t *read_len, const uint32_t *read_first_line, uint32_t n_reads, msgpu_graph **out);
/* The same WITHOUT the copy: the four tables are borrowed (e.g. the pinned result of msgpu_overlap_batched; the EdgeMatch
 * table alone is 0.8 GB on BASELINE.json configs[2]) and must stay valid and unchanged until msgpu_graph_free. */
int  msgpu_graph_create_borrowed(const msgpu_edge *edges, uint64_t n_edges, const msgpu_edgematch *ems, uint64_t n_ems,
                                 const msgpu_order *orders, uint64_t n_orders, const uint32_t *ids, uint64_t n_ids,
                                 const int32_t *read_len, const uint32_t *read_first_line, uint32_t n_reads,
                                 msgpu_graph **out);
void msgpu_graph_free(msgpu_graph *g);
const char *msgpu_graph_last_error(const msgpu_graph *g);
/* rows (optional): the VertexMatch table, for contract()'s "getVertexMatch(start, id) != nullptr" (main.cpp:514-519);
 * NULL = every id of an order has one (true for tables produced by this library). */
int msgpu_graph_clean_up(msgpu_graph *g, const int64_t *contraction_order, const msgpu_row *rows, size_t n_rows);
/* host threads for msgpu_graph_linearize (components are independent, cf. one assemblePaths job per component,
 * src/main.cpp:300-310); default 1; the result does not depend on it */
int msgpu_graph_set_threads(msgpu_graph *g, uint32_t n_threads);
int msgpu_graph_linearize(msgpu_graph *g);
int msgpu_graph_get_stats(const msgpu_graph *g, msgpu_graph_stats *out);
uint32_t msgpu_graph_path_count(const msgpu_graph *g);
/* After msgpu_graph_linearize: the edge-table index of the edge under every path step, paths concatenated in path order
 * (path i contributes n_reads_i - 1 entries); owned by the graph.  With a graph created without an EdgeMatch table, hand
 * this list to msgpu_get_edgematches and its result to msgpu_graph_set_path_edgematches (copied) before
 * msgpu_graph_path_input, which fails with MSGPU_E_STATE until then. */
int msgpu_graph_path_edges(const msgpu_graph *g, const uint32_t **edge_idx, size_t *n);
int msgpu_graph_set_path_edgematches(msgpu_graph *g, const uint64_t *em_off, const msgpu_edgematch *ems);
/* path i (asm_idx = i) as assemblePath input; pointers are owned by the graph and valid until msgpu_graph_free;
 * rows / n_rows are left empty (use msgpu_assembly_set_rows). */
int msgpu_graph_path_input(const msgpu_graph *g, uint32_t i, msgpu_path_input *out);
/* msgpu_graph_path_input for every path + msgpu_assembly_add_paths in one call (status: msgpu_graph_path_count(g) entries
 * or NULL): the assemblePaths fan-out of src/main.cpp:620-677 over the paths of this graph.  The graph must outlive the
 * call (the layouts read its tables), not the assembly. */
int msgpu_assembly_add_graph_paths(msgpu_assembly *a, const msgpu_graph *g, uint32_t n_threads, int *status);
/* inspection (all optional): per vertex alive flag and direction (1 e_POS / 0 e_NEG / 2 e_NONE); per edge (table
 * order) alive flag, consensus direction (same coding) and weight */
int msgpu_graph_state(const msgpu_graph *g, uint8_t *vertex_alive, uint8_t *vertex_direction, uint8_t *edge_alive,
                      uint8_t *edge_consensus, uint64_t *edge_weight);

/* The graph primitives of the stage on caller-supplied graphs (vertices 0 .. n_vertices-1, edge i = (a[i], b[i])): the
 * same code msgpu_graph_clean_up / msgpu_graph_linearize run, exposed so that the vectors the reference's own unit tests
 * hold for them can be replayed through this boundary (tests/golden/ref_tests/).  consensus: 1 e_POS, 0 e_NEG, 2 e_NONE.
 *   getMaxSpanTree          libms/src/kernel/mst.cpp:75-111   (libms/tests/MST_test.cpp:8-60)
 *   getConnectedComponents  libms/src/kernel/cc.cpp:33-70     (libms/tests/CC_test.cpp:11-90)
 *   GraphUtil::getShortestPath  include/ms/graph/Graph.h:927-978  (libms/tests/Graph_test.cpp:279-331); directed != 0:
 *                           a DiGraph (edges a -> b, neighbours = successors)
 *   DiGraph::sortTopologically  libms/src/graph/Graph.cpp:359-395 (libms/tests/Graph_test.cpp:393-423) */
int msgpu_graph_max_span_tree(uint32_t n_vertices, const uint32_t *a, const uint32_t *b, const uint64_t *weight,
                              const uint8_t *consensus, uint64_t n_edges, uint8_t *in_tree /* n_edges */);
/* Graph / DiGraph bookkeeping on its own -- what the clean-up's deletions (src/main.cpp:243,259,286) and the component split
 * (src/main.cpp:625 getSubgraph) rest on; the reference's tests hold vectors for it (libms/tests/Graph_test.cpp:81-277,
 * 333-391: EdgeDeletion, VertexDeletion, Neighboor, Subgraph, Degree).  A flat graph of n_vertices and the pairs (a[i], b[i])
 * -- undirected, or a -> b when directed != 0; a pair given twice is ONE edge, as Graph::addEdge has it (Graph.cpp:212-230) --
 * is built by the stage's CSR builder; `ops` is run over it in order, with tombstones as the stage keeps them; every query
 * appends to `out`:
 *   MSGPU_GOP_DELETE_EDGE x y    Graph::deleteEdge (Graph.cpp:187-210); nothing when there is no such edge
 *   MSGPU_GOP_DELETE_VERTEX x    Graph::deleteVertex (:158-185): the vertex and every edge at it
 *   MSGPU_GOP_ORDER / _SIZE      getOrder() / getSize()                                   -> 1 word
 *   MSGPU_GOP_HAS_EDGE x y       hasEdge (undirected: either way round)                   -> 0 | 1
 *   MSGPU_GOP_NEIGHBORS x        getNeighbors (undirected) / getSuccessors (directed)     -> count, then the ids ascending
 *   MSGPU_GOP_PREDECESSORS x     getPredecessors (directed only)                          -> count, ids
 *   MSGPU_GOP_IN_DEGREE x / _OUT_DEGREE x   getInDegrees().at(x) / getOutDegrees().at(x)  -> 1 word (0xffffffff: x was deleted)
 *   MSGPU_GOP_SUBGRAPH x y       getSubgraph of the y vertices listed in ops[x .. x + y) (entries MSGPU_GOP_ARG, .x = vertex)
 *                                                                                         -> order, size, then (a, b) per edge
 * *n_out = words the script produces; MSGPU_E_ARG when they do not fit out_capacity (call again with room) or an operand is
 * out of range. */
typedef struct msgpu_graph_op {
  uint32_t op, x, y;
} msgpu_graph_op;
#define MSGPU_GOP_DELETE_EDGE 1u
#define MSGPU_GOP_DELETE_VERTEX 2u
#define MSGPU_GOP_ORDER 3u
#define MSGPU_GOP_SIZE 4u
#define MSGPU_GOP_HAS_EDGE 5u
#define MSGPU_GOP_NEIGHBORS 6u
#define MSGPU_GOP_PREDECESSORS 7u
#define MSGPU_GOP_IN_DEGREE 8u
#define MSGPU_GOP_OUT_DEGREE 9u
#define MSGPU_GOP_SUBGRAPH 10u
#define MSGPU_GOP_ARG 11u
int msgpu_graph_bookkeeping(uint32_t n_vertices, const uint32_t *a, const uint32_t *b, uint64_t n_edges, int directed,
                            const msgpu_graph_op *ops, size_t n_ops, uint32_t *out, size_t out_capacity, size_t *n_out);
int msgpu_graph_connected_components(uint32_t n_vertices, const uint32_t *a, const uint32_t *b, const uint8_t *consensus,
                                     uint64_t n_edges, uint32_t *component /* n_vertices */, uint32_t *n_components);
/* *n_path: in = capacity of path, out = vertices on the path (0 = unreachable); MSGPU_E_ARG when it does not fit */
int msgpu_graph_shortest_path(uint32_t n_vertices, const uint32_t *a, const uint32_t *b, uint64_t n_edges, int directed,
                              uint32_t src, uint32_t dst, uint32_t *path, uint32_t *n_path);
/* order: n_vertices entries of room; *n_order < n_vertices when the graph has a cycle (its vertices never appear) */
int msgpu_graph_sort_topologically(uint32_t n_vertices, const uint32_t *a, const uint32_t *b, uint64_t n_edges,
                                   uint32_t *order, uint32_t *n_order);

/* ---- banded edit distance (no reference counterpart) ---------------------------------
 * The meter for north_star's "consensus sequences within a stated edit-distance tolerance": Levenshtein distance
 * (unit costs, global) of n pairs a[a_off .. a_off+a_len) vs b[b_off .. b_off+b_len) taken from two DEVICE buffers,
 * inside the band |j - i| <= band (band <= 127).  out[p] (host) = the distance when it is <= band, else band + 1
 * (= min(distance, band + 1): a path of d <= band edits never leaves the band).  Sequences shorter than 2^30 bytes.
 * Computed by furthest-reaching points per (edits, diagonal); MSGPU_ED_DP=1 in the environment selects the banded
 * anti-diagonal DP kernel instead (same numbers, for cross-checks). */
typedef struct msgpu_align_pair {
  uint64_t a_off, b_off;
  uint32_t a_len, b_len;
} msgpu_align_pair;
int msgpu_edit_distance(msgpu_seqctx *ctx, const void *d_a, const void *d_b, const msgpu_align_pair *pairs, size_t n,
                        uint32_t band, uint32_t *out);
/* The edit script of every pair beside its distance ("unitig-to-read mapping", rule 10, is the definition).  Arguments and
 * limits as above.  dist[p] is what msgpu_edit_distance returns.  off has n + 1 entries; pair p owns
 * words[off[p] .. off[p + 1]): d + 1 words for a pair within the band, none for a capped pair.  Word t < d is
 * kind << 30 | run with the kinds 1 = X, 2 = D (a base of a only), 3 = I (a base of b only), in forward order, run = the
 * number of '=' columns in front of that edit; word d is kind 0 with the trailing '=' run.  When the words do not fit
 * capacity: MSGPU_E_ARG with dist, off and *n_words set, so that the caller can call again with room.  MSGPU_E_STATE: a
 * table on the device contradicted its pair's distance (a defect of the kernels, counted and reported, never passed over).
 * MSGPU_ALIGN_SLOTS=<n> in the environment lowers the number of tables that pairs of more than 31 edits share. */
int msgpu_edit_script(msgpu_seqctx *ctx, const void *d_a, const void *d_b, const msgpu_align_pair *pairs, size_t n,
                      uint32_t band, uint32_t *dist, uint64_t *off /* n + 1 */, uint32_t *words, uint64_t capacity,
                      uint64_t *n_words);
/* Rule 11's extension of every pair on its own ("unitig-to-read mapping", rule 11.2 to 11.4, is the definition): a and b
 * are the flanks A and B, lengths below 2^29.  flags bit 0 = reversed: a_off and b_off then name the byte BEHIND the flank,
 * whose byte i is base[off - 1 - i]; every other bit must be 0.  ends[p] is the end cell; off has n + 1 entries and pair p
 * owns words[off[p] .. off[p + 1]), e + 1 words in msgpu_edit_script's format, in the flank's own order.  Capacity as
 * msgpu_edit_script: MSGPU_E_ARG with ends, off and *n_words set when the words do not fit.  MSGPU_E_STATE: a table
 * contradicted itself on the walk (a defect of the kernel, counted and reported, never passed over). */
int msgpu_extend_ends(msgpu_seqctx *ctx, const void *d_a, const void *d_b, const msgpu_align_pair *pairs, size_t n,
                      uint32_t band, uint32_t flags, msgpu_ext_end *ends, uint64_t *off /* n + 1 */, uint32_t *words,
                      uint64_t capacity, uint64_t *n_words);

/* ---- assembly evaluation (no reference counterpart) ---------------------------------------------
 * Consensus QV and completeness of an assembly from the k-mers of the accurate short reads, without a reference genome:
 * the k-mer spectrum of the reads against the k-mers of the assembly, which is Merqury's method.  Merqury is not part of the
 * reference tree: the stage is defined by the rules below and is checked without tolerance, on integers, against their
 * restatement in plain Python (tests/ev_oracle.py).  Parameters: k (1..64), min_count (1..10000, default 2, the unitig
 * stage's default; anything else is MSGPU_E_ARG), intervals (rule 7, 0 = off).
 *  1. Read k-mers.  These follow the k-mer abundance filter's rules for FASTQ, for windows (k in 1..64, case folded, any
 *     byte outside ACGTacgt breaks the windows that hold it) and for canonical keys, error code, file and line included.
 *     The two cases are one file, and two files, which may have different record counts (the unitig stage's msgpu_pair
 *     semantics).  R(x) is the exact number of windows of the read files whose canonical k-mer is x.
 *  2. Assembly k-mers.  A window is k consecutive bases of one FASTA record, with the same alphabet rule.  It never crosses
 *     two records.  A(x) is the number of assembly windows whose canonical k-mer is x (its copy number).  A window with
 *     R(x) = 0 is missing.
 *  3. Per record and in total.  The figures are length, windows, missing.  A record shorter than k has 0 windows.
 *  4. QV.  This is host arithmetic in double precision from the two integers (msgpu_ev_qv).  With p = missing / windows,
 *     the error rate is e = -expm1(log1p(-p) / k).  This form avoids cancellation for small p.
 *     qv = -10 * log10(e) + 0.0, so that e = 1 prints 0.00, never -0.00.  missing = 0 gives +inf (text inf).
 *     windows = 0 gives no value (NaN, text -).
 *  5. Spectrum.  S[c][a] is the number of distinct canonical k-mers x with copy class c = min(A(x), 4) and read
 *     abundance a.  a is 0 for assembly-only k-mers; there c >= 1.  Otherwise a = min(R(x), 10001); row 10001 is the
 *     filter's cap row.  That makes 5 x 10002 counters.  For every a >= 1 the sum over c is the filter's histogram row.
 *  6. Completeness.  This is host arithmetic on the spectrum for the parameter min_count.  solid is the sum of S[c][a] over
 *     a >= min_count and all c.  found is the same sum over c >= 1.
 *  7. Error intervals, on request.  One interval is made per maximal run of consecutive missing windows of a record.  A
 *     run of windows s..e gives (record, s, e + k).  Intervals are not merged, so two runs separated by one present window
 *     give two intervals that overlap.  They are ordered by record, then start.  A run never continues into the next record.
 *  8. Report text.  It is tab-separated.  The first line is "#k <k> min_count <m>" (MSGPU_EV_TEXT_HEAD).  Per assembly
 *     (MSGPU_EV_TEXT_REPORT): a line "#assembly <file name>" (the path's last component), then the header
 *     "record length windows missing qv", then one line per record in file order; the name is the record name up to the
 *     first blank; qv is printed with %.2f.  Then a line "total ...", and a line
 *     "completeness <found> <solid> <100 * found / solid with %.4f, or - when solid = 0>".  MSGPU_EV_TEXT_SPECTRUM holds
 *     the lines "a c0 c1 c2 c3 c4" for the rows that are not all zero, MSGPU_EV_TEXT_BED the lines "name start end"; each
 *     of the two opens with the "#assembly" line as well, so that the texts of several assemblies can follow one another.
 *  9. Limits.  Each is an error that names the figure, never a fault.  At most 2^30 distinct read k-mers (the hash table
 *     over them has 2^31 slots at most).  Fewer than 2^31 assembly windows: the bases of an assembly, as its store holds
 *     them, stay below 2^31 (a 3 Gb genome is out of scope).  The file limits of the filter and of the sequence store.
 *     Everything resident together within the budget, else MSGPU_E_NOMEM naming the sizes.
 * The table of the reads (sorted distinct keys, R, an open-addressing table over them) is a handle of its own: it is made
 * once, from files or from a resident msgpu_pair, and serves any number of assemblies, as msgpu_map_index serves the mapper.
 * A run reads it; the only array of it a run writes is the per-key assembly count A, which the run zeroes itself.  A context
 * holds one table at a time (a second one is MSGPU_E_STATE until the first is freed), and a table of another context, or a
 * pair on another device than the context's, is MSGPU_E_ARG. */
typedef struct msgpu_evctx msgpu_evctx; /* a device context of the stage */
typedef struct msgpu_ev_table msgpu_ev_table;
typedef struct msgpu_ev_result msgpu_ev_result;
#define MSGPU_EV_CLASSES 5u    /* copy classes 0..4 */
#define MSGPU_EV_ROWS 10002u   /* read abundance 0..10001 */
typedef struct msgpu_ev_params {
  int32_t  k;
  uint32_t min_count; /* rule 6 */
  uint32_t intervals; /* rule 7: 0 = off */
  uint32_t reserved;
} msgpu_ev_params;
void        msgpu_ev_default_params(msgpu_ev_params *p); /* k = 21, min_count = 2, intervals = 0 */
int         msgpu_ev_create(int device, msgpu_evctx **out); /* MSGPU_E_NODEVICE without a GPU */
void        msgpu_ev_destroy(msgpu_evctx *ctx);
const char *msgpu_ev_last_error(const msgpu_evctx *ctx);
uint64_t    msgpu_ev_error_line(const msgpu_evctx *ctx); /* after MSGPU_E_FORMAT: the 1-based line of a read file */
int         msgpu_ev_error_file(const msgpu_evctx *ctx); /* after MSGPU_E_FORMAT / MSGPU_E_IO: read file 0 or 1 */
/* Rule 4 on its own: host only, no device.  MSGPU_E_ARG for k outside 1..64 or missing > windows. */
int         msgpu_ev_qv(uint64_t missing, uint64_t windows, int k, double *qv);
typedef struct msgpu_ev_tstats {
  uint64_t n_records[2], bytes_in[2];
  uint64_t n_windows, n_distinct, largest_partition;
  uint64_t bytes_resident;  /* keys, R, A and the hash table */
  uint32_t k, n_partitions;
  float load_ms, records_ms; /* host wall, as msgpu_kf_stats */
  float bins_ms, extract_ms, sort_ms, runs_ms, select_ms; /* the count, device by events */
  float table_ms;            /* gather, sort and the hash table (host wall) */
  float wall_ms;
  uint32_t reserved;
} msgpu_ev_tstats;
/* The table of one (path_b NULL) or two read files, or of a pair opened by msgpu_kf_open_pair.  budget_bytes bounds the
 * count's partition buffers as in msgpu_kf_run (0: half of the free device memory). */
int         msgpu_ev_table_open(msgpu_evctx *ctx, int k, const char *path_a, const char *path_b, uint64_t budget_bytes,
                                msgpu_ev_table **out);
int         msgpu_ev_table_open_pair(msgpu_evctx *ctx, int k, const msgpu_pair *pair, uint64_t budget_bytes, msgpu_ev_table **out);
int         msgpu_ev_table_stats(const msgpu_ev_table *table, msgpu_ev_tstats *out);
void        msgpu_ev_table_free(msgpu_ev_table *table);
typedef struct msgpu_ev_record { /* rule 3, in file order */
  uint64_t length, windows, missing;
} msgpu_ev_record;
typedef struct msgpu_ev_interval { /* rule 7 */
  uint64_t start, end;
  uint32_t record, reserved;
} msgpu_ev_interval;
typedef struct msgpu_ev_stats {
  uint64_t n_records, n_bases, n_windows, n_missing;
  uint64_t n_missing_distinct;  /* distinct assembly-only k-mers: the sum of row a = 0 */
  uint64_t n_intervals;
  uint64_t solid, found;        /* rule 6 */
  uint64_t n_lost_publications; /* scalar read-backs that had to fall back to a copy */
  uint64_t bytes_peak;          /* the run's own device memory, the table and the store not counted */
  uint32_t k, min_count;
  float load_ms;                /* the assembly into its store (host wall) */
  float window_ms;              /* the window kernel, device by events from here on */
  float reduce_ms;              /* the per-record sums */
  float missing_ms;             /* sort and run lengths of the missing keys, row a = 0 */
  float spectrum_ms, intervals_ms, copy_ms;
  float host_ms;                /* the texts (wall) */
  float wall_ms;
  uint32_t reserved;
} msgpu_ev_stats;
/* One assembly on a table.  params->k must be the table's.  flags must be 0.  Synchronous; tables and texts are kept in
 * the result. */
int         msgpu_ev_run_table(msgpu_evctx *ctx, const msgpu_ev_params *params, msgpu_ev_table *table, const char *assembly_path,
                               uint32_t flags, msgpu_ev_result **out);
/* table_open + run_table + table_free */
int         msgpu_ev_run(msgpu_evctx *ctx, const msgpu_ev_params *params, const char *path_a, const char *path_b,
                         const char *assembly_path, uint32_t flags, uint64_t budget_bytes, msgpu_ev_result **out);
int         msgpu_ev_result_stats(const msgpu_ev_result *r, msgpu_ev_stats *out);
int         msgpu_ev_result_records(const msgpu_ev_result *r, const msgpu_ev_record **records, const msgpu_ev_record **total, uint64_t *n);
/* MSGPU_EV_CLASSES rows of MSGPU_EV_ROWS counters: S[c][a] = spectrum[c * MSGPU_EV_ROWS + a] */
int         msgpu_ev_result_spectrum(const msgpu_ev_result *r, const uint64_t **spectrum);
int         msgpu_ev_result_intervals(const msgpu_ev_result *r, const msgpu_ev_interval **intervals, uint64_t *n);
#define MSGPU_EV_TEXT_HEAD 0
#define MSGPU_EV_TEXT_REPORT 1
#define MSGPU_EV_TEXT_SPECTRUM 2
#define MSGPU_EV_TEXT_BED 3 /* empty unless params->intervals */
const char *msgpu_ev_result_text(const msgpu_ev_result *r, int which, uint64_t *len);
void        msgpu_ev_result_free(msgpu_ev_result *r);

#ifdef __cplusplus
}
#endif
#endif /* MSGPU_H */
