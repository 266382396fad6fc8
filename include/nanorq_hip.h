/*
 * nanorq_hip.h -- thin C ABI into the gfx950 (MI355X) RaptorQ precode-solve / symbol-generation
 * path.  Plain C types only: device and host pointers as void*, sizes, int status returns
 * (0 = ok, negative = error, text via nrq_ctx_error()); no C++ exceptions cross this line.
 *
 * This is the seam the drop-in library (include/nanorq.h, include/io.h) sits on, and the
 * entry points a binding of the reference would call instead of its CPU solver.  Reference
 * interfaces replaced (file:line in sleepybishop/nanorq):
 *   precode_matrix_gen / precode_matrix_invert / precode_matrix_intermediate   include/precode.h:10-12
 *   nanorq_generate_symbols  (load + plan + replay)                            lib/nanorq.c:206-232
 *   nanorq_repair_block      (patch + plan + replay + regenerate gaps)         lib/nanorq.c:591-631
 *   decode_row / nanorq_encode (LT symbol generation)                          lib/nanorq.c:184-204, :403-435
 *   oblas oaxpy/oscal/oswaprow row kernels (absent submodule deps/oblas)       precode.c:7,18,20
 * The unit of work is a batch of independent source blocks of equal (K, T) that stay resident in
 * HBM; persistent workgroups solve one 16/8/4/2-byte column strip of one block at a time out of LDS.
 */
#ifndef NANORQ_HIP_H
#define NANORQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nrq_ctx nrq_ctx;

/* statistics of the last encode/decode call (host side, for benchmarks and tests) */
typedef struct nrq_call_stats {
  double plan_ms;      /* symbolic stage wall time (all blocks) */
  double host_ms;      /* whole host side of the call before the launch returns */
  uint32_t strip_bytes;/* column-strip width chosen (16/12/8/4/2) */
  uint32_t lds_bytes;  /* dynamic LDS per workgroup */
  uint32_t grid;       /* (persistent) workgroups launched */
  uint32_t planner;    /* 0 = host planner, 1 = device planner */
  uint64_t plan_bytes; /* plan bytes resident on the device for this call */
  uint64_t xor_ops;    /* row XOR ops in the forward passes, summed over blocks */
  uint32_t npiv, u, nlev, nfree; /* of block 0 */
  uint32_t wg_threads; /* threads per workgroup of the solve launch */
  uint32_t strips_per_slot; /* strips a work slot holds (a whole 128-byte line group unless work is scarce) */
  uint32_t wg_waves_per_simd; /* register budget of the solve kernel variant launched: waves per SIMD it was compiled for */
  uint32_t host_planned; /* decode blocks whose plan exceeded a device-planner capacity and was rebuilt on the host */
  uint32_t movers_aligned; /* 1: the solve kernel variant without byte-wise paths in its movers (all rows aligned, T a multiple of the strip) */
  uint32_t plan_ahead;  /* 1: the decode found its planner run already issued (nrq_decode_plan_ahead) */
  uint32_t strip_bytes_b, blocks_b; /* the batch's SECOND block list: blocks whose LDS image does not fit at strip_bytes run in a launch
                                     * of their own at this narrower width (0 / 0: one list) */
  uint32_t plan_wg_threads;  /* decode: threads per workgroup of the planner kernel run (1024 / 256 / 128; 0: planned on the host) */
  uint32_t plan_compact_state; /* 1: that run took the planner instance that keeps the peeling state in the workspace (big blocks) */
  uint32_t plan_segmented;   /* 1: that run was segmented into parts (the biggest blocks) */
  uint32_t backsub_strip;    /* bytes per strip of the back-substitution kernel after a narrow-strip solve (32 / 16; 0: no split) */
  uint32_t encplan_device;   /* encode: the plan in use was built by the planner kernel (else by the host planner) */
  uint32_t out_view;         /* decode: jobs of the call launched with the W' image of their lists (nrq_job out_w != 0: no back-substitution) */
  uint32_t need_view;        /* decode without intermediate symbols: device-planned jobs of the call launched on the needed-pivot view (the
                              * plan has one and no W' image: the back-substitution takes the pivots the missing symbols' lists name) */
  uint32_t nneed;            /* the needed pivots of the first such job's plan (a subset of its npiv pivots) */
  uint32_t plan_scan_lists;  /* decode: device-planned blocks of the call whose missing symbols' lists the planner laid out in row order by
                              * its prefix scan (more missing symbols than its frontier queues hold lengths of; nrq_plan_hdr scan_lists) */
} nrq_call_stats;

/* One context per GPU (one process per GPU: no cross-device state).  `stream` is a hipStream_t the
 * caller owns (NULL = the default stream); all work of later calls is enqueued on it. */
int nrq_ctx_create(int device, void *stream, nrq_ctx **out);
void nrq_ctx_destroy(nrq_ctx *ctx);
int nrq_ctx_set_stream(nrq_ctx *ctx, void *stream);
const char *nrq_ctx_error(nrq_ctx *ctx);
int nrq_ctx_sync(nrq_ctx *ctx);
void nrq_ctx_last_stats(nrq_ctx *ctx, nrq_call_stats *out);
/* where decode plans are built: 1 = on the GPU (default; planner kernel, one workgroup per block),
 * 0 = on the host (thread pool).  The environment variable NRQ_HOST_PLANNER=1 selects 0 at creation. */
int nrq_ctx_set_planner(nrq_ctx *ctx, int device_planner);
/* Tuning / test knobs of the launch path by option name: the rows of NRQ_KNOBS in nanorq_amd/csrc/launch_shape.h (field, default,
 * the NRQ_* environment variable that sets the same field when the context is created, option name, meaning).  An unknown name
 * returns -1.  Results never depend on a knob, only speed and which kernel variant runs.
 * Fault injection for tests: "fail_after" n -- the n-th checked runtime call of the context from now on (allocation, copy,
 * event / stream operation, the error check behind a launch) is not made and fails instead, once (0 = off);
 * "faults_injected" returns the number of failures injected so far.  "fail_after" exists only on a context created with
 * NANORQ_HIP_FAULT_INJECT=1 in the environment (else: unknown option, -1), and not at all in a -DNRQ_NO_FAULT_INJECT build. */
int nrq_ctx_set_option(nrq_ctx *ctx, const char *name, long long value);
/* threads used for host-side planning (0 = hardware concurrency) */
int nrq_ctx_set_threads(nrq_ctx *ctx, int n);

/* Parameters of RFC 6330 section 5.3.1.2 for K source symbols: out = {K',J,S,H,W,L,P,P1,U,B}. */
int nrq_params(uint32_t K, uint32_t out[10]);

/* In every call below K is the number of source symbols of a block and Kp the RFC 6330 Table 2 row (K')
 * it is coded with: 0 = the row the RFC assigns to K; nanorq passes block 0's K' for every block of an
 * object (lib/nanorq.c:289, :372), which can exceed a short block's own row.
 *
 * Build (or fetch the cached) plan for encoding blocks of K symbols: the counterpart of
 * nanorq_precalculate (lib/nanorq.c:393-401).  Implied by nrq_encode_blocks. */
int nrq_precalculate(nrq_ctx *ctx, uint32_t K, uint32_t Kp);
/* First-use costs of blocks of (K, K') paid now instead of inside the first encode / decode: the code object is loaded, the
 * per-K' constants are built and uploaded, and with encode_plan != 0 the encode plan is built (1: enqueued, for big K', as by
 * nrq_precalculate; 2: waited for).  The object layer calls it from nanorq_encoder_new* / nanorq_decoder_new* -- the reference pays nothing
 * comparable (its tables are static), so the constructors are where a drop-in can put it without a timed call seeing it. */
int nrq_warm(nrq_ctx *ctx, uint32_t K, uint32_t Kp, int encode_plan);
/* drop cached encode plans (so that a benchmark can time plan generation) */
void nrq_plan_cache_clear(nrq_ctx *ctx);

/* Encode nblk source blocks (asynchronous on the context's stream).
 *   d_src    device: block b at d_src + b*src_stride, source symbol j at + j*T        (K*T bytes)
 *   d_inter  device or NULL: block b's L intermediate symbols at d_inter + b*inter_stride
 *   h_esis   host: nrep repair ESIs (each K <= esi < 2^24), the same list for every block
 *   d_rep    device: block b's repair symbol q at d_rep + b*rep_stride + q*T
 * Bit-exact with nanorq_generate_symbols + nanorq_encode(esi) of the reference. */
int nrq_encode_blocks(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, const void *d_src, size_t src_stride,
                      void *d_inter, size_t inter_stride, uint32_t nrep, const uint32_t *h_esis, void *d_rep,
                      size_t rep_stride);

/* Decode nblk source blocks (asynchronous on the context's stream; h_status is final on return).
 *   d_src    device, in/out: block b at d_src + b*src_stride; received source symbols are in place at
 *            row esi, rows of missing symbols are overwritten with the recovered symbols
 *   h_lost   host: missing source ESIs of block b, ascending, at h_lost[b*lost_cap .. + h_nlost[b])
 *   h_rep_esi host: ESIs (>= K) of block b's received repair symbols in ARRIVAL order at
 *            h_rep_esi[b*rep_cap .. + h_nrep[b]); symbol q at d_rep + b*rep_stride + q*T.  Any ESI up to 2^24 - 1, in any
 *            order; an ESI < K (or >= 2^24) fails the block, which is left untouched.  An ESI may repeat: the copy adds no
 *            rank, so verdict and bytes are those of the list without it (as nanorq_decoder_add_symbol drops it)
 *   d_inter  device or NULL: intermediate symbols out
 *   h_status host out: 1 = block recovered, 0 = not decodable (fewer repair symbols than gaps, or
 *            rank deficient: the caller may add symbols and retry, as with nanorq_repair_block)
 * The i-th missing ESI takes the i-th repair symbol, surplus symbols become extra constraint rows
 * (lib/nanorq.c:527-565). */
int nrq_decode_blocks(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, void *d_src, size_t src_stride,
                      const uint32_t *h_lost, const uint32_t *h_nlost, uint32_t lost_cap, const uint32_t *h_rep_esi,
                      const uint32_t *h_nrep, uint32_t rep_cap, const void *d_rep, size_t rep_stride, void *d_inter,
                      size_t inter_stride, int *h_status);

/* Same, using spare symbols only when needed.  Block b's system is first built from its first h_nrep[b]
 * repair symbols (>= h_nlost[b]); if it is rank deficient the planner takes further symbols from the list,
 * one at a time up to h_nrep_avail[b], as additional constraint rows -- on the GPU without redoing the
 * elimination -- instead of failing.  This is what a receiver does that calls nanorq_repair_block again
 * after one more packet (lib/nanorq.c:620-623), minus the second pass.  h_nrep_avail may be NULL (= h_nrep);
 * h_used (nullable) receives the number of repair symbols each recovered block consumed. */
int nrq_decode_blocks_lazy(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, void *d_src, size_t src_stride,
                           const uint32_t *h_lost, const uint32_t *h_nlost, uint32_t lost_cap, const uint32_t *h_rep_esi,
                           const uint32_t *h_nrep, const uint32_t *h_nrep_avail, uint32_t rep_cap, const void *d_rep,
                           size_t rep_stride, void *d_inter, size_t inter_stride, int *h_status, uint32_t *h_used);

/* Issue the planner run of a later nrq_decode_blocks / nrq_decode_blocks_lazy call now (same arguments, without the result
 * arrays): the symbolic stage (reference precode_matrix_invert's planning half, lib/precode.c:347-377) needs the reception
 * pattern only, not the symbols, so it can run on the planner stream while earlier batches are still being solved.  The
 * decode call with identical arguments then only waits for it (nrq_call_stats::plan_ahead = 1).  Up to two runs may be waiting
 * (-6 beyond that); they are consumed in the order they were issued: a decode call discards the runs in front of the one
 * issued for it (and all of them if none was).  Two runs issued back to back execute side by side (two planner streams, two workspaces, three sets of
 * plan arenas): a planner workgroup is latency bound on one compute unit, so a pipeline that keeps two batches' plans in
 * flight gets them at twice the rate.  Not for the per-block-address variants (_v, _vc). */
int nrq_decode_plan_ahead(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, void *d_src, size_t src_stride,
                          const uint32_t *h_lost, const uint32_t *h_nlost, uint32_t lost_cap, const uint32_t *h_rep_esi,
                          const uint32_t *h_nrep, const uint32_t *h_nrep_avail, uint32_t rep_cap, const void *d_rep, size_t rep_stride,
                          void *d_inter, size_t inter_stride);

/* nrq_encode_blocks (no repair symbols) with block b's intermediate symbols going to device address d_inter_v[b]. */
int nrq_encode_blocks_v(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, const void *d_src, size_t src_stride,
                        const uint64_t *d_inter_v);
/* nrq_decode_blocks_lazy for blocks that do not lie at a fixed stride: block b's source rows at device address
 * d_src_v[b], its repair symbols at d_rep_v[b] (host arrays of device addresses).  No intermediate symbols out. */
int nrq_decode_blocks_v(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, const uint64_t *d_src_v, const uint32_t *h_lost,
                        const uint32_t *h_nlost, uint32_t lost_cap, const uint32_t *h_rep_esi, const uint32_t *h_nrep,
                        const uint32_t *h_nrep_avail, uint32_t rep_cap, const uint64_t *d_rep_v, int *h_status, uint32_t *h_used);

/* nrq_decode_blocks_v that also writes the intermediate symbols: block b's L symbols go to device address d_inter_v[b] (a host array of
 * device addresses; NULL: none, and the call IS nrq_decode_blocks_v).  As in every decode that is given a place for them, all
 * pivots are back-substituted (the needed-pivot view applies only without intermediate symbols); a block that is not recovered
 * leaves its L * T bytes undefined.  What nrq_rx_decode calls while a relay is attached to the reception. */
int nrq_decode_blocks_vi(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, const uint64_t *d_src_v, const uint32_t *h_lost,
                         const uint32_t *h_nlost, uint32_t lost_cap, const uint32_t *h_rep_esi, const uint32_t *h_nrep,
                         const uint32_t *h_nrep_avail, uint32_t rep_cap, const uint64_t *d_rep_v, const uint64_t *d_inter_v, int *h_status,
                         uint32_t *h_used);

/* nrq_decode_blocks_v with ONE planner run for all blocks and the solve in chunks of `chunk_blocks` blocks, in order: after
 * chunk i has been solved the event chunk_done[i] (nrq_event_new; ceil(nblk / chunk_blocks) of them) is recorded on the
 * context's stream, so that a caller can start moving the first blocks (nrq_stream_wait on a copy stream) while the later
 * ones are still being solved -- the planner's fixed cost (a launch the host waits for, ~3 ms) is paid once, not per chunk.
 * The events are valid once the call has RETURNED (the caller enqueues its waits afterwards): with the host planner, or when
 * blocks had to be re-planned on the host, all chunks are solved by one later launch and every event is recorded behind that;
 * on a negative return value the events are undefined.
 * upload_done (nullable): events the solve of chunk i waits for before it reads the chunk's symbols (their upload).
 * Replaces nanorq_repair_block per block (reference lib/nanorq.c:591-631). */
int nrq_decode_blocks_vc(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, const uint64_t *d_src_v, const uint32_t *h_lost,
                         const uint32_t *h_nlost, uint32_t lost_cap, const uint32_t *h_rep_esi, const uint32_t *h_nrep,
                         const uint32_t *h_nrep_avail, uint32_t rep_cap, const uint64_t *d_rep_v, int *h_status, uint32_t *h_used,
                         uint32_t chunk_blocks, void *const *chunk_done, void *const *upload_done);

/* Generate encoding symbols from intermediate symbols already in HBM (after encode/decode with
 * d_inter != NULL): symbol q of block b = LT(C_b, isi[q]) -> d_out + b*out_stride + q*T.
 * h_isi are INTERNAL symbol ids (esi for esi < K, esi + K' - K for repair symbols). */
int nrq_gen_symbols(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, const void *d_inter, size_t inter_stride,
                    uint32_t n, const uint32_t *h_isi, void *d_out, size_t out_stride);

/* the same with the list of internal symbol ids already in device memory (enqueue only: nothing is staged, nothing waited for;
 * a pipeline that generates the same symbols for block after block uploads the list once) */
int nrq_gen_symbols_dev(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, const void *d_inter, size_t inter_stride,
                        uint32_t n, const uint32_t *d_isi, void *d_out, size_t out_stride);

/* Raw device memory helpers for hosts without a HIP binding of their own (the drop-in C library and
 * the ctypes tests use them; PyTorch callers pass tensor data pointers instead). */
int nrq_dev_alloc(nrq_ctx *ctx, size_t bytes, void **out);
int nrq_dev_free(nrq_ctx *ctx, void *p);
int nrq_dev_upload(nrq_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);   /* synchronous */
int nrq_dev_download(nrq_ctx *ctx, void *h_dst, const void *d_src, size_t bytes); /* synchronous */
int nrq_dev_memset(nrq_ctx *ctx, void *d_dst, int value, size_t bytes);
/* enqueue-only variants (ordered on the context's stream; complete after nrq_ctx_sync) */
int nrq_dev_upload_async(nrq_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int nrq_dev_download_async(nrq_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int nrq_dev_copy(nrq_ctx *ctx, void *d_dst, const void *d_src, size_t bytes); /* device to device, enqueue-only */

/* nrq_dev_alloc / nrq_dev_free come out of a caching pool of the context (no hipMalloc / hipFree per call, no
 * synchronisation on free); nrq_dev_trim hands the cached blocks back to the driver. */
int nrq_dev_trim(nrq_ctx *ctx);
/* nrq_dev_free refuses (-1) an address that is no block of the context and a block that is already cached (a second free).
 * The pool's books, for tests: out[0] blocks the pool owns (handed out or cached), out[1] blocks cached, out[2] bytes cached. */
int nrq_dev_pool_books(nrq_ctx *ctx, size_t out[3]);

/* ---- what the object layer's streaming path is made of (reference: transfer_esi / load_symbol_matrix,
 * lib/nanorq.c:148-182, and the seek+read/write loops of lib/io.c behind them) ----
 * Page-locked host memory: the copy engines move it at PCIe speed and asynchronously. */
int nrq_host_alloc_pinned(size_t bytes, void **out);
void nrq_host_free_pinned(void *p);
int nrq_host_register(void *p, size_t bytes);   /* page-lock caller memory in place */
void nrq_host_unregister(void *p);
int nrq_host_is_pinned(const void *p);          /* 1 if p lies in page-locked (allocated or registered) host memory */
int nrq_host_range_is_pinned(const void *p, size_t bytes); /* 1 if all of [p, p + bytes) does (ends + a probe every 2 MiB) */
/* Copies and ordering on the context's streams.  `stream`: 0 = the context's stream (kernels), 1 = its upload stream,
 * 2 = its download stream.  Everything is enqueue-only; events order the streams among each other. */
int nrq_copy_on(nrq_ctx *ctx, int stream, void *dst, const void *src, size_t bytes); /* direction from the pointers */
int nrq_memset_on(nrq_ctx *ctx, int stream, void *d_dst, int value, size_t bytes);
int nrq_event_new(nrq_ctx *ctx, void **out);
void nrq_event_free(void *ev);
int nrq_event_record(nrq_ctx *ctx, void *ev, int stream);
int nrq_stream_wait(nrq_ctx *ctx, int stream, void *ev);  /* later work on `stream` waits for ev */
int nrq_event_sync(nrq_ctx *ctx, void *ev);                /* the host waits */
int nrq_stream_sync(nrq_ctx *ctx, int stream);
/* Symbol ingestion on the device: symbol k (T bytes at d_blob + k*T, device memory) is copied to device address
 * h_dst[k] (0 = skip) -- received packets go up in one piece and are put into their rows by a kernel. */
int nrq_scatter_symbols(nrq_ctx *ctx, int stream, const void *d_blob, uint32_t n, uint32_t T, const uint64_t *h_dst);
/* Control data (KBs to a few MB, a multiple of 16 bytes, both ends 16-byte aligned) from page-locked host memory into a device
 * buffer by a kernel that reads the host memory itself: unlike a copy it does not queue behind the bulk uploads the copy
 * engine is busy with.  stream selector as in nrq_copy_on, plus 3 = the stream of the sorting kernels. */
int nrq_ctl_copy(nrq_ctx *ctx, int stream, void *d_dst, const void *h_pinned, size_t bytes);
/* the same with the destination addresses already on the device (enqueue only: no staging of the list, nothing waited for) */
int nrq_scatter_symbols_dev(nrq_ctx *ctx, int stream, const void *d_blob, uint32_t n, uint32_t T, const uint64_t *d_dst);

/* Rows by address pair (enqueue only): row k, T bytes, from address d_pairs[2k] to address d_pairs[2k+1] (0 = skip); either side
 * may be page-locked host memory the device can address.  The receiver's repaired symbols go from their device rows straight to
 * their places in the caller's page-locked output buffer this way (nanorq_repair_all): no staging, no copy per row. */
int nrq_move_rows_dev(nrq_ctx *ctx, int stream, const uint64_t *d_pairs, uint32_t n, uint32_t T);
/* the address at which a kernel reaches page-locked host memory (hipHostMalloc'ed or hipHostRegister'ed); 0 = it cannot */
uint64_t nrq_host_device_address(const void *p);

/* ---- device-resident receiver: packets that are already in device memory (a GPU-direct NIC, another kernel's output, a peer
 * copy) are classified, placed into their rows and booked on the GPU; only the reception pattern comes down, to the planner ----
 * A reception is nblk blocks of equal (K, K', T) with SBNs sbn0 .. sbn0+nblk-1 (an object with two block classes is two
 * receptions fed from the same packets).  Block b's source row e lies at src + b*src_stride + e*T, its repair row q at
 * rep + b*rep_stride + q*T; d_src / d_rep NULL: allocated from the context's pool (strides K*T and rep_cap*T).  max_esi 0 = 2*K'
 * (the object layer's default); rep_cap: repair rows per block.  Kp 0 = the row RFC 6330 assigns to K.
 * A reception belongs to its context and is destroyed before it. */
typedef struct nrq_rx nrq_rx;
#define NRQ_RX_TAG_INLINE 1u /* nrq_rx_add flag: each packet starts with the RFC 6330 section 3.2 FEC Payload ID (SBN 8 bits, ESI 24
                              * bits, network byte order); its payload follows at +4 */
#define NRQ_RX_FULL 3        /* result code beside NANORQ_SYM_*: a repair symbol that found the block's rep_cap rows used (not marked seen) */
int nrq_rx_create(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, uint32_t sbn0, uint32_t max_esi, uint32_t rep_cap,
                  void *d_src, size_t src_stride, void *d_rep, size_t rep_stride, nrq_rx **out);
void nrq_rx_destroy(nrq_rx *rx);
/* Ingest n packets (enqueue only, on the context's stream): packet k at d_pkts + k*pkt_stride, its tag (nanorq_tag() form) at
 * d_tags[k], or in the packet with NRQ_RX_TAG_INLINE (d_tags NULL; pkt_stride >= T + 4).  Each packet of the reception's blocks
 * gets the code nanorq_decoder_add_symbol would give it, in packet order (ERR: ESI > max_esi; IGN: the block has no source gaps;
 * DUP: the ESI was seen, in an earlier call or earlier in this one; else ADDED, or NRQ_RX_FULL) into d_results[k] (device,
 * nullable); packets of other SBNs and their result entries are left untouched.  An added source symbol goes to row esi, an
 * added repair symbol to the block's next repair row: the repair list is in arrival (packet) order. */
int nrq_rx_add(nrq_rx *rx, const void *d_pkts, size_t pkt_stride, const uint32_t *d_tags, uint32_t n, uint32_t flags, int32_t *d_results);
/* per block: missing source symbols and repair rows used (waits for the work enqueued before) */
int nrq_rx_counts(nrq_rx *rx, uint32_t *h_nlost, uint32_t *h_nrep);
/* the same plus the lists (each nullable): block b's missing source ESIs, ascending, at h_lost[b*K ..], its repair ESIs in
 * arrival order at h_rep_esi[b*rep_cap ..] (waits) */
int nrq_rx_lists(nrq_rx *rx, uint32_t *h_nlost, uint32_t *h_nrep, uint32_t *h_lost, uint32_t *h_rep_esi);
/* Decode the reception's blocks in place (nrq_decode_blocks_v on the compact lists: the planner, its host fallback and the
 * lazy use of spare symbols as in every decode).  h_status[b]: 1 = the block is complete (nothing was missing, or recovered:
 * later packets for it are IGN, as after nanorq_repair_block), 0 = not decodable yet (too few repair symbols, too many for the
 * rows beyond L, or rank deficient: ingest more and decode again).  h_used (nullable): repair symbols a recovered block used.
 * h_status is final on return; the solve is enqueued on the context's stream. */
int nrq_rx_decode(nrq_rx *rx, int *h_status, uint32_t *h_used);
void *nrq_rx_src(nrq_rx *rx);
void *nrq_rx_rep(nrq_rx *rx);
int nrq_rx_reset(nrq_rx *rx); /* forget everything received (enqueue only); the rows keep their bytes */
/* What the reception HOLDS: the symbols whose bytes lie in its rows -- per block its seen source symbols (after a decode: all K)
 * and its repair rows in use; a symbol that got NRQ_RX_FULL is not held, and after nrq_rx_reset nothing is.  *h_n = their number,
 * sum over the blocks of K - nlost + nrep (waits for the work enqueued before, as nrq_rx_counts).  d_tags (device, nullable) with
 * cap >= *h_n receives their tags (nanorq_tag() form), listed on the device: block-major, within a block the source ESIs
 * ascending, then the repair ESIs in arrival order; cap too small: -1, *h_n still filled.  Only *h_n is final on return: the
 * writing of d_tags is enqueued on the context's stream behind the wait, so later work on that stream (an emit) sees the tags,
 * while a read from the host or from another stream needs nrq_ctx_sync first.  It is the list a relay's NRQ_TX_HELD emit writes
 * in full (below). */
int nrq_rx_held(nrq_rx *rx, uint32_t *d_tags, uint32_t cap, uint32_t *h_n);
/* What the reception WANTS: the tags (nanorq_tag() form) it asks upstream for to top its blocks up, listed on the device -- the
 * NACK of a node in a distribution tree, in the form nrq_tx_emit / nrq_otx_emit take (with or without NRQ_TX_HELD), so the loop
 * want -> emit -> add -> decode runs without a host-built list.  Per block b, with g = its missing source symbols (nlost of
 * nrq_rx_counts) and r = its repair rows in use, min(nrep, rep_cap):
 *   g == 0 (complete: nothing was missing, or a decode recovered it): nothing, in either mode.
 *   flags == NRQ_WANT_SOURCE: the g source ESIs < K whose seen bit is clear, ascending -- the symbols a parent relay that is not
 *     ready can still give under NRQ_TX_HELD where it holds them, and a sender gives as plain row copies.  extra and esi_from
 *     must be 0 (-1).
 *   flags == 0 (repair symbols): need = max(g + extra - r, 0), capped at the free repair rows rep_cap - r (a symbol beyond them
 *     would only come back NRQ_RX_FULL); the list is the `need` lowest ESIs e with max(K, esi_from) <= e <= max_esi whose seen bit
 *     is clear, ascending -- shorter if the range holds fewer, empty if esi_from > max_esi.  A repair ESI's seen bit is set only
 *     when the symbol was ADDED: one that got NRQ_RX_FULL is asked for again, which is intended.  extra > 2^24: -1.
 *   any other flag bit: -1.
 * Tags are ((sbn0 + b) << 24) | e, block-major in SBN order.  The list depends on the reception's books alone: the same books
 * give the same list.
 * extra is the overhead wanted beyond g received symbols (0, 1 or 2 in practice).  RANK DEFICIENCY: a block that nrq_rx_decode
 * left at status 0 although r >= g has enough symbols but not enough independent ones; the reception keeps no decode verdicts, so
 * such a block wants nothing until the caller raises extra above its surplus r - g (ask again with extra = r - g + 1 or more).
 * The price on the other blocks is at most extra symbols each.  esi_from keeps the requests of a node with several parents, or
 * to a parent that already runs a carousel, in disjoint ESI ranges.
 * The calling contract is nrq_rx_held's: the call waits for the work enqueued before it and *h_n, the total, is final on return;
 * d_tags NULL counts only; cap < *h_n: -1, *h_n still filled, nothing written; else the writing of d_tags is enqueued on the
 * context's stream, so an emit enqueued behind it sees the tags without a host wait (a read from the host or from another stream
 * needs nrq_ctx_sync first).  The call only reads the reception's books; after nrq_rx_reset every block wants all of itself. */
#define NRQ_WANT_SOURCE 1u
int nrq_rx_want(nrq_rx *rx, uint32_t flags, uint32_t extra, uint32_t esi_from, uint32_t *d_tags, uint32_t cap, uint32_t *h_n);

/* ---- device-resident sender: packets (an optional FEC Payload ID and a payload, at a packet stride) written straight into
 * device memory -- for a GPU-direct NIC, or a kernel that sends from device memory -- for any list of (SBN, ESI) ----
 * A transmission is nblk blocks of equal (K, K', T) with SBNs sbn0 .. sbn0+nblk-1 (an object with two block classes is two
 * transmissions).  Block b's source row e lies at d_src + b*src_stride + e*T (src_stride 0 = K*T); the source rows are read by
 * nrq_tx_encode AND by every emit (a source packet is a copy of its row), so they must stay unchanged until the last emit has
 * completed.  The intermediate symbols (nblk * L * T bytes) come from the context's pool.  Kp 0 = the row RFC 6330 assigns to K.
 * Every call is enqueue-only on the context's stream; a transmission belongs to its context and is destroyed before it.
 * The payload of (SBN, ESI) is bit-exact with nanorq_encode (ESI < K: source row ESI; else LT(C, ESI + K' - K)). */
typedef struct nrq_tx nrq_tx;
#define NRQ_TX_TAG_INLINE 1u /* packet = the RFC 6330 section 3.2 FEC Payload ID (SBN 8 bits, ESI 24 bits, network byte order), then the
                              * payload at +4 (pkt_stride >= T + 4) */
#define NRQ_TX_HELD 2u       /* tag-list emits of a relay: a block that is not ready still gives the symbols its reception holds (below) */
#define NRQ_TX_NOT_READY (-2) /* emit result code beside 0 and -1: a block of a relay that is not ready (the packet is left untouched) */
int nrq_tx_create(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, uint32_t sbn0, const void *d_src, size_t src_stride,
                  nrq_tx **out);
void nrq_tx_destroy(nrq_tx *tx);
/* solve every block (nrq_encode_blocks): the intermediate symbols into the transmission's own buffer; emits before it: -1 */
int nrq_tx_encode(nrq_tx *tx);
/* Packet k for tag d_tags[k] (nanorq_tag() form, device memory) at d_pkts + k*pkt_stride (pkt_stride >= T, + 4 inline).
 * d_results (device, nullable): 0 = written, -1 = SBN outside the transmission (the packet is left untouched); a relay also gives
 * NRQ_TX_NOT_READY (the table in the relay section).  flags: NRQ_TX_TAG_INLINE, and on a relay NRQ_TX_HELD (a sender: -1). */
int nrq_tx_emit(nrq_tx *tx, const uint32_t *d_tags, uint32_t n, void *d_pkts, size_t pkt_stride, uint32_t flags, int32_t *d_results);
/* ESIs esi0 .. esi0+n-1 of EVERY block (n * nblk packets, no tag list): order 0 = block-major (packet k -> block k / n, ESI
 * esi0 + k % n), 1 = interleaved (packet k -> block k % nblk, ESI esi0 + k / nblk); d_tags_out (device, nullable) receives each
 * packet's tag. */
int nrq_tx_emit_range(nrq_tx *tx, uint32_t esi0, uint32_t n, int order, void *d_pkts, size_t pkt_stride, uint32_t flags,
                      uint32_t *d_tags_out);
void *nrq_tx_inter(nrq_tx *tx); /* block b's L intermediate symbols at + b*L*T (valid after nrq_tx_encode) */
/* per block (nblk entries): 1 = its packets can be emitted.  A sender: all 1 after nrq_tx_encode, all 0 before; a relay: below. */
int nrq_tx_ready(nrq_tx *tx, uint32_t *h_ready);

/* ---- relay: a transmission made FROM a reception, over the reception's own rows -- the node in the middle of a distribution tree,
 * which receives blocks and goes on sending them, fresh repair symbols included, without solving a block twice ----
 * The result is an ordinary nrq_tx (same emit calls, same destroy) whose source rows are the reception's, in place, and whose
 * intermediate symbols (nblk * L * T bytes) come from the context's pool.  One relay per reception (a second call: -1).  Destroy
 * the relay before its reception; a reception destroyed first detaches the relay, whose later calls fail with an error text.
 * A block of the relay is READY when it is complete in the reception and its intermediate symbols are written:
 *   - from the moment the relay is attached, nrq_rx_decode writes the intermediate symbols of every block it recovers into the
 *     relay's buffer (nrq_decode_blocks_vi: all pivots are back-substituted), and the block is ready when the call returns;
 *   - nrq_tx_encode on a relay makes ready every complete block that is not: it solves, with the encoder, only the blocks that
 *     completed without a decode (nothing was missing) or were decoded before the relay was attached, leaves ready blocks alone
 *     and launches nothing when there is nothing to do.  It may be called any number of times, after any decode (it waits for
 *     the reception's counts);
 *   - nrq_rx_reset makes every block not ready.
 * nrq_tx_emit on a relay is never refused for want of an encode: a packet of a block that is not ready is left untouched and
 * gets NRQ_TX_NOT_READY in d_results (-1 keeps meaning "SBN outside the span").  nrq_tx_emit_range needs every block ready
 * (-1 and a text that names the blocks that are not).  Everything is enqueued on the context's stream, so an emit enqueued
 * after a decode sees that decode's rows and intermediate symbols; a ready block never changes again (later packets for it are
 * IGN), so its packets stay valid while the reception takes packets for other blocks.
 *
 * Held symbols (NRQ_TX_HELD, nrq_tx_emit / nrq_otx_emit on a relay): a block that is not ready -- short of symbols, rank
 * deficient, or decoded before the relay was attached -- still answers with the symbols the reception holds, so a relay can cut
 * through (forward a batch as soon as it is ingested), serve a NACK from a partial block and hand all it has to a late child.
 * The packet of (SBN, ESI), and its entry of d_results:
 *   SBN outside the span                                         untouched   -1
 *   block ready                                                  any ESI, as without the flag   0
 *   block not ready, ESI < K, the source symbol is held          a copy of source row ESI       0
 *   block not ready, ESI >= K, the repair symbol is held         a copy of its repair row       0
 *   block not ready, the symbol is not held (or no NRQ_TX_HELD)   untouched   NRQ_TX_NOT_READY
 * "Held" is nrq_rx_held's meaning: ADDED by nrq_rx_add (not NRQ_RX_FULL, not after a reset), or a source row a decode recovered.
 * A held packet has the bytes that were ingested, hence those of nanorq_encode.  nrq_rx_decode reads the repair rows and their
 * ESI list and leaves both as they are, so held repair symbols stay valid after a decode (a block decoded before the relay was
 * attached gives all K source symbols and its received repair symbols, but no fresh ones until nrq_tx_encode); a held symbol's
 * row does not change until a reset, and source rows change only where they were missing.  The emit is enqueue-only and sees
 * the symbols of every nrq_rx_add enqueued before it, without a host wait.  Without the flag every call is as it was;
 * nrq_tx_emit_range and nrq_otx_emit_all refuse it (-1: their packet maps are analytic over all blocks). */
int nrq_rx_relay(nrq_rx *rx, nrq_tx **out);

/* ---- whole objects (RFC 6330 section 4.4.1.2) on the device: an object of F bytes and its OTI, sent and received through the
 * sender and receiver above without the caller partitioning it ----
 * The object is Z source blocks: ZL blocks of KL symbols (SBN 0 .. ZL-1), then ZS of KS (SBN ZL .. Z-1); each block is coded
 * with K' = KpL / KpS (block 0's row for both classes unless NANORQ_EXT_PER_BLOCK_KP).  A symbol of T bytes is N sub-symbols,
 * NL of TL bytes then NS of TS bytes; sub-block j of block b is one stretch of K_b * T_j bytes of the object, and row e of the
 * block is the concatenation of row e of its sub-blocks (nanorq_api.c's symbol_offset).  Bytes of the object at offset >= F
 * read as zero.  These are the parameters nanorq_encoder_new_ext / nanorq_decoder_new_ext derive, computed without a GPU. */
typedef struct nrq_obj_params {
  uint64_t F;
  uint32_t T, Al, Z, N, Kt;
  uint32_t ZL, KL, KpL;  /* first block class (ZL may be 0) */
  uint32_t ZS, KS, KpS;  /* second block class */
  uint32_t NL, TL, NS, TS; /* sub-blocks: NL of TL bytes, then NS of TS bytes (NL may be 0) */
  uint32_t flags;        /* NANORQ_EXT_* */
  uint32_t max_esi;      /* 2 * K' of block 0, the decoder's default */
  uint64_t oti_common;   /* nanorq_oti_common / nanorq_oti_scheme_specific of such an object */
  uint32_t oti_specific;
} nrq_obj_params;
/* the parameters of nanorq_encoder_new_ext(F, T, K, Z, N, Al, flags); -1 where it returns NULL */
int nrq_obj_params_enc(uint64_t F, uint32_t T, uint32_t K, uint32_t Z, uint32_t N, uint32_t Al, uint32_t flags, nrq_obj_params *out);
/* the parameters of nanorq_decoder_new_ext(common, specific, flags); -1 where it returns NULL */
int nrq_obj_params_oti(uint64_t common, uint32_t specific, uint32_t flags, nrq_obj_params *out);

/* The layout step alone (enqueue only): to_obj 0 = the object (F bytes at d_obj) into the blocks' row images (Kt * T bytes at d_rows,
 * block b's at + its object offset; bytes past F read as zero), 1 = the row images into the object (nothing at or past F written). */
int nrq_obj_layout(nrq_ctx *ctx, const nrq_obj_params *prm, void *d_obj, void *d_rows, int to_obj);

/* Object sender.  d_obj: the object, F bytes of device memory, as it is.  N = 1: the blocks are read in place, only a last block
 * that the object does not fill is staged (zero-padded) in the context's pool; N > 1: the blocks' row images are laid out from the
 * object into the pool by a kernel.  In both cases the object must stay unchanged until the last emit has completed.
 * Every call but create / destroy / oti is enqueue-only on the context's stream; the sender belongs to its context. */
typedef struct nrq_otx nrq_otx;
int nrq_otx_create(nrq_ctx *ctx, const nrq_obj_params *prm, const void *d_obj, nrq_otx **out);
void nrq_otx_destroy(nrq_otx *tx);
int nrq_otx_encode(nrq_otx *tx); /* every block (nrq_encode_blocks per class); emits before it: -1 */
/* Packet k for tag d_tags[k] over all blocks of the object, as nrq_tx_emit (payloads bit-exact with nanorq_encode of
 * nanorq_encoder_new_ext with the same arguments); d_results[k]: 0 written, -1 SBN >= Z (packet left untouched). */
int nrq_otx_emit(nrq_otx *tx, const uint32_t *d_tags, uint32_t n, void *d_pkts, size_t pkt_stride, uint32_t flags, int32_t *d_results);
/* ESIs 0 .. K_b + nrep - 1 of every block b (its source symbols, then nrep repair symbols): sum_b (K_b + nrep) packets.
 * order 0 = block-major (block 0's packets, then block 1's, ...), 1 = interleaved (the pairs (sbn, i) with i < K_sbn + nrep
 * sorted by (i, sbn)).  d_tags_out (device, nullable) receives each packet's tag. */
int nrq_otx_emit_all(nrq_otx *tx, uint32_t nrep, int order, void *d_pkts, size_t pkt_stride, uint32_t flags, uint32_t *d_tags_out);
int nrq_otx_oti(nrq_otx *tx, uint64_t *common, uint32_t *specific);
int nrq_otx_ready(nrq_otx *tx, uint32_t *h_ready); /* as nrq_tx_ready, Z entries */

/* Object receiver: the blocks' row images in the context's pool, one reception (nrq_rx) per block class, both with the
 * object's max_esi.  rep_cap: repair rows per block. */
typedef struct nrq_orx nrq_orx;
int nrq_orx_create(nrq_ctx *ctx, const nrq_obj_params *prm, uint32_t rep_cap, nrq_orx **out);
void nrq_orx_destroy(nrq_orx *rx);
/* as nrq_rx_add over the whole object: every packet gets the code nanorq_decoder_add_symbol of a decoder made from the same OTI
 * and flags would give it, in packet order, or NRQ_RX_FULL.  (SBN >= Z: NANORQ_SYM_ERR for an ESI above max_esi, else
 * NANORQ_SYM_IGN -- the object layer's block of no symbols.) */
int nrq_orx_add(nrq_orx *rx, const void *d_pkts, size_t pkt_stride, const uint32_t *d_tags, uint32_t n, uint32_t flags, int32_t *d_results);
int nrq_orx_counts(nrq_orx *rx, uint32_t *h_nlost, uint32_t *h_nrep); /* Z entries each */
int nrq_orx_held(nrq_orx *rx, uint32_t *d_tags, uint32_t cap, uint32_t *h_n); /* as nrq_rx_held, over both block classes in SBN order */
/* as nrq_rx_want, over both block classes in SBN order: each class with its own K, esi_from applies to both */
int nrq_orx_want(nrq_orx *rx, uint32_t flags, uint32_t extra, uint32_t esi_from, uint32_t *d_tags, uint32_t cap, uint32_t *h_n);
int nrq_orx_decode(nrq_orx *rx, int *h_status, uint32_t *h_used);    /* as nrq_rx_decode, Z entries */
/* every complete block into d_out (F bytes, device) in the object's layout; bytes past F and the bytes of incomplete blocks are
 * left untouched.  Returns the number of blocks still incomplete (>= 0), or < 0 on error.  Waits for the counts, enqueues the
 * copy. */
int nrq_orx_write(nrq_orx *rx, void *d_out);
/* The object's relay (as nrq_rx_relay, over both block classes): an ordinary nrq_otx whose table lies over the receiver's row
 * images -- class L at their start, class S behind it, each with its own K' under NANORQ_EXT_PER_BLOCK_KP; the Kt * T bytes of
 * the row images make a staged last block unnecessary, and neither nrq_orx_write nor a layout pass is on the forwarding path --
 * and whose intermediate symbols (ZL * L_L * T + ZS * L_S * T bytes) come from the context's pool.  nrq_orx_decode feeds it,
 * nrq_otx_encode makes the remaining complete blocks ready, nrq_otx_emit gives NRQ_TX_NOT_READY per packet (and takes NRQ_TX_HELD,
 * answering from the symbols either class's reception holds), nrq_otx_emit_all needs every block ready, nrq_otx_oti returns
 * the object's OTI.  Packets are bit-exact with those of nrq_otx_create over the original object.  Destroy it before the
 * receiver (else it is detached). */
int nrq_orx_relay(nrq_orx *rx, nrq_otx **out);

/* ---- packets of several symbols (RFC 6330 section 4.4.2) ----
 * A packet may carry up to G symbols (1 <= G <= NRQ_PKT_SYMS_MAX) of ONE source block, all source or all repair, with consecutive
 * ESIs: packet k has a first tag (SBN, e_k) -- d_tags[k], or the inline FEC Payload ID -- and a count c_k; symbol i < c_k has ESI
 * e_k + i (in ESI space: the SBN never changes inside a packet, an ESI above 2^24 - 1 does not exist) and its payload at
 * hdr + i * T in the packet (hdr = 0, or 4 with the tag inline); pkt_stride >= hdr + G * T.  Slot (k, i) has index k * G + i; the
 * EXPANSION of a packet list is its one-symbol packets in slot order.  d_nsym (device, uint8 per packet, nullable) gives the
 * counts; NULL is the sender's rule: c_k = G, except that a packet whose first ESI is below the block's K carries
 * min(G, K - e_k) (each block class of an object with its own K).
 *
 * nrq_rx_add_syms / nrq_orx_add_syms: as nrq_rx_add / nrq_orx_add.  d_results (nullable) has n * G entries: slot (k, i), i < c_k,
 * gets the code nrq_rx_add gives that symbol in the expansion (a duplicate inside the list and the ERR of an ESI above max_esi
 * included; a symbol whose ESI would pass 2^24 - 1 is ERR); slots i >= c_k and the slots of SBNs outside the reception are left
 * untouched.  A receiver is liberal: a given count 1..G is taken as it is, also where the packet runs from source into repair
 * ESIs.  A given count of 0 or above G is malformed: slot k * G gets ERR, nothing of the packet is booked, its other slots are
 * untouched.  (Object form, SBN >= Z: c slots get ERR / IGN as in nrq_orx_add, c = d_nsym[k], or G without d_nsym; a count of 0
 * or above G gives slot k * G ERR there too.)
 * After the call the reception is in exactly the state nrq_rx_add leaves after the expansion -- seen bits, gaps, repair rows and
 * their ESIs in arrival order, source rows -- so counts, lists, decode, held, want and relays need nothing new.  G = 1 with
 * d_nsym NULL is nrq_rx_add.  Refused (-1 and a text, nothing enqueued): G outside 1..NRQ_PKT_SYMS_MAX, a stride too small,
 * n * G > 0x7FFFFFFF, an unknown flag, d_tags together with (or without either of) NRQ_RX_TAG_INLINE.
 *
 * nrq_tx_emit_syms / nrq_otx_emit_syms: as nrq_tx_emit / nrq_otx_emit.  A written packet is the FEC Payload ID of (SBN, e_k)
 * when inline, then c_k payloads, each byte for byte what nrq_tx_emit writes for that (SBN, ESI); the bytes of the packet behind
 * hdr + c_k * T are untouched.  d_results[k] (n entries, nullable): 0 written; -1 SBN outside the span; NRQ_TX_NOT_READY a relay's
 * block that is not ready; NRQ_TX_BAD_RANGE a count of 0 or above G, a GIVEN count that takes a packet starting below K to K or
 * beyond (a sender is strict), or e_k + c_k - 1 > 0xFFFFFF -- in all but the first case the packet is untouched.  Admission is
 * per packet (every symbol of a packet has the packet's block): no packet is ever half written.
 * NRQ_TX_HELD (a relay or an object's relay only; a sender refuses it, -1): packet k = (SBN, e, c) of a block that is NOT ready,
 * with an admissible range, is written iff the reception holds EVERY symbol e .. e+c-1 (nrq_rx_held's meaning) -- all or nothing,
 * so that the flag leaves no packet half written either: 0 and the header if inline, then c payloads, payload i byte for byte what
 * nrq_tx_emit with NRQ_TX_HELD writes for (SBN, e+i) at that moment; else NRQ_TX_NOT_READY and the packet untouched.  An
 * inadmissible range (above) is NRQ_TX_BAD_RANGE whether or not the block is ready; a ready block and an SBN outside the span are
 * as without the flag.  c is d_nsym[k], or the sender's rule.  The list nrq_rx_held_syms gives is answered in full.
 *
 * nrq_tx_emit_range_syms / nrq_otx_emit_all_syms: ESIs esi0 .. esi0+n-1 (0 .. K+nrep-1) of every block, packetised per block: the
 * source run [esi0, min(K, esi0+n)) cut into packets of G from its start, the last one short, then the repair run
 * [max(K, esi0), esi0+n) likewise -- nrq_pkt_count(K, esi0, n, G) packets per block.  order 0: block-major; order 1: round j holds
 * packet j of every block that has one, in SBN order (a class with fewer packets drops out of the later rounds).  d_tags_out
 * (first tags) and d_nsym_out (counts), both nullable, are in packet order.  *h_npkt (nullable) receives the number of packets.
 * A relay with a block that is not ready is refused, as nrq_tx_emit_range; so is NRQ_TX_HELD.
 *
 * nrq_rx_want_syms / nrq_rx_held_syms (and nrq_orx_*): what nrq_rx_want / nrq_rx_held list for the same reception and the same
 * flags, extra, esi_from, as PACKETS of up to G symbols: d_tags[k] a first tag, d_nsym[k] its count -- the form nrq_tx_emit_syms
 * takes (d_tags, d_nsym) and nrq_rx_add_syms takes (d_nsym).  The PACKETISATION of the one-symbol list L of one block, in L's
 * order: a RUN is a maximal stretch L[i..j] with L[i+m] == L[i] + m (consecutive ESIs in list order); a run never holds both an ESI
 * below K and one at or above K (the source part and the repair part of a held list are packetised apart, also where ESI K - 1 is
 * followed by ESI K); every run is cut into packets of G from its START, the last one short.  The packetisation of a listing is
 * that of its blocks, one behind the other (SBN order; an object: class L, then class S, each with its own K).  Its expansion is
 * L word for word; with G = 1 the first tags are L and every count is 1.
 *   want, repair mode    the truncation at the block's `need` only shortens the tail: the last packet may be cut short by it
 *   held, source part    the seen source ESIs ascending
 *   held, repair part    arrival order: a run is rep_esi[q+1] == rep_esi[q] + 1, it lies in consecutive repair rows (arrival 12, 13,
 *                        14 is one packet (12, 3); arrival 14, 13, 12 is three packets of 1)
 * The calling contract is nrq_rx_want's: the call waits for the work enqueued before it; *h_npkt (required) is the number of
 * packets, *h_nsym (nullable) the number of symbols -- exactly the one-symbol call's *h_n -- both final on return and from ONE
 * wait; d_tags and d_nsym both NULL: the counts only; cap is in packets, cap < *h_npkt gives -1 with both totals still filled and
 * nothing written; otherwise the writing is enqueued on the context's stream, so an emit behind it sees the list without a host
 * wait.  The calls only read the reception's books.  Refused (-1 and a text, nothing enqueued): what nrq_rx_want refuses, G
 * outside 1..NRQ_PKT_SYMS_MAX, exactly one of d_tags / d_nsym given, h_npkt NULL.
 *
 * Reception sets and sender sets take such packets through nrq_rxset_add_syms and nrq_txset_emit_syms (below, behind the sets). */
#define NRQ_PKT_SYMS_MAX 64u
#define NRQ_TX_BAD_RANGE (-3)
uint32_t nrq_pkt_count(uint32_t K, uint32_t esi0, uint32_t n, uint32_t G);
int nrq_rx_add_syms(nrq_rx *rx, const void *d_pkts, size_t pkt_stride, const uint32_t *d_tags, uint32_t n, uint32_t G, const uint8_t *d_nsym,
                    uint32_t flags, int32_t *d_results);
int nrq_orx_add_syms(nrq_orx *rx, const void *d_pkts, size_t pkt_stride, const uint32_t *d_tags, uint32_t n, uint32_t G, const uint8_t *d_nsym,
                     uint32_t flags, int32_t *d_results);
int nrq_tx_emit_syms(nrq_tx *tx, const uint32_t *d_tags, uint32_t n, uint32_t G, const uint8_t *d_nsym, void *d_pkts, size_t pkt_stride,
                     uint32_t flags, int32_t *d_results);
int nrq_otx_emit_syms(nrq_otx *tx, const uint32_t *d_tags, uint32_t n, uint32_t G, const uint8_t *d_nsym, void *d_pkts, size_t pkt_stride,
                      uint32_t flags, int32_t *d_results);
int nrq_tx_emit_range_syms(nrq_tx *tx, uint32_t esi0, uint32_t n, uint32_t G, int order, void *d_pkts, size_t pkt_stride, uint32_t flags,
                           uint32_t *d_tags_out, uint8_t *d_nsym_out, uint32_t *h_npkt);
int nrq_otx_emit_all_syms(nrq_otx *tx, uint32_t nrep, uint32_t G, int order, void *d_pkts, size_t pkt_stride, uint32_t flags,
                          uint32_t *d_tags_out, uint8_t *d_nsym_out, uint32_t *h_npkt);
int nrq_rx_want_syms(nrq_rx *rx, uint32_t flags, uint32_t extra, uint32_t esi_from, uint32_t G, uint32_t *d_tags, uint8_t *d_nsym, uint32_t cap,
                     uint32_t *h_npkt, uint32_t *h_nsym);
int nrq_orx_want_syms(nrq_orx *rx, uint32_t flags, uint32_t extra, uint32_t esi_from, uint32_t G, uint32_t *d_tags, uint8_t *d_nsym, uint32_t cap,
                      uint32_t *h_npkt, uint32_t *h_nsym);
int nrq_rx_held_syms(nrq_rx *rx, uint32_t G, uint32_t *d_tags, uint8_t *d_nsym, uint32_t cap, uint32_t *h_npkt, uint32_t *h_nsym);
int nrq_orx_held_syms(nrq_orx *rx, uint32_t G, uint32_t *d_tags, uint8_t *d_nsym, uint32_t cap, uint32_t *h_npkt, uint32_t *h_nsym);

/* ---- reception sets:the packets of MANY receptions in one buffer, ingested in one pass ----
 * A set is a table of member receptions of one context and one T, each under a 32-bit KEY the caller chooses (a TOI, a flow
 * number): a tag names (SBN, ESI) and nothing more, the key names the reception or object the SBN belongs to.  nrq_rxset_add
 * runs the passes of nrq_rx_add once over all packets with the table in device memory, where today R receptions fed from one
 * buffer cost R scans (and an object of two block classes two and a half).  Members stay ordinary receptions: nrq_rx_add /
 * nrq_orx_add on a member between two set calls, counts, lists, decode, reset, held, want and relays work on the same books.
 * The caps follow from the kernels: one LDS counter per block in the histogram pass and four in the classify pass (4 KB + 16 KB at
 * 1024 blocks), 4 B x blocks x tiles of scratch, a linear search over the members per packet. */
typedef struct nrq_rxset nrq_rxset;
#define NRQ_RXSET_MAX_MEMBERS 64u   /* receptions (an object with two classes counts twice) */
#define NRQ_RXSET_MAX_BLOCKS  1024u /* blocks over all members */
#define NRQ_RX_KEY_INLINE 2u        /* with NRQ_RX_TAG_INLINE: packet = key (32 bits, network byte order), FEC Payload ID, payload at +8 */
int nrq_rxset_create(nrq_ctx *ctx, uint32_t T, nrq_rxset **out);
void nrq_rxset_destroy(nrq_rxset *set); /* members live on, detached */
/* Attach a reception, or an object receiver (both block classes, and the SBN >= Z rule of nrq_orx_add), under `key`.  Refused
 * (-1, nrq_ctx_error): another context; a T that is not the set's; a reception that is in a set already; a (key, SBN span) that
 * overlaps a member's (the same span under another key is fine, so is another span under the same key); for an object, any other
 * member under its key, and any further member under an object's key -- an object owns its key; a cap exceeded.  Attach and
 * detach wait for the context's stream (the table lives in device memory).  Destroying a member that is still attached detaches
 * it first. */
int nrq_rxset_attach(nrq_rxset *set, uint32_t key, nrq_rx *rx);
int nrq_rxset_attach_obj(nrq_rxset *set, uint32_t key, nrq_orx *orx);
int nrq_rxset_detach(nrq_rxset *set, uint32_t key); /* every member under key; unknown key: -1 */
/* Ingest n packets (enqueue only, on the context's stream).  Packets and tags as in nrq_rx_add; packet k's key is d_keys[k]
 * (device), or lies in the packet in front of the FEC Payload ID with NRQ_RX_KEY_INLINE | NRQ_RX_TAG_INLINE (d_keys and d_tags
 * NULL; pkt_stride >= T + 8), or is 0 for every packet (d_keys NULL without the flag).  Every member ends with what nrq_rx_add on
 * it alone gives for exactly the packets that carry its key, in packet order: the same codes in the same entries of d_results
 * (device, nullable), the same rows, the same repair list in arrival order, the same counts and seen bits.  A packet with an
 * attached object's key and SBN >= Z gets what nrq_orx_add gives it (ERR above max_esi, else IGN).  A packet that belongs to no
 * member -- an unknown key, or a known key that is no object's with an SBN outside its members -- keeps its d_results entry
 * untouched, and nothing of it is copied.  n == 0 and an empty set: 0.  Errors (-1): those of nrq_rx_add, NRQ_RX_KEY_INLINE
 * without NRQ_RX_TAG_INLINE, NRQ_RX_KEY_INLINE with d_keys. */
int nrq_rxset_add(nrq_rxset *set, const void *d_pkts, size_t pkt_stride, const uint32_t *d_keys, const uint32_t *d_tags, uint32_t n,
                  uint32_t flags, int32_t *d_results);
/* ---- counts, lists and decode of ALL members in one call ----
 * The block order of a set: members sorted by (key, first SBN), a member's blocks in SBN order -- an attached object is its Z
 * blocks in SBN order under its key.  The order depends on the membership alone, not on the order of the attach calls, and
 * changes only with attach, detach and a member's destruction.  Every per-block array below is in this order.
 *
 * nrq_rxset_blocks: entry j = (key, SBN) of block j.  *h_n = the number of blocks; h_keys / h_sbn nullable (both NULL: the
 * number only); cap < *h_n with an array given: -1, *h_n still filled.  Host state only: no wait, no launch. */
int nrq_rxset_blocks(nrq_rxset *set, uint32_t *h_keys, uint32_t *h_sbn, uint32_t cap, uint32_t *h_n);
/* nrq_rx_counts over all members: one gather kernel over the member table, one download, one wait. */
int nrq_rxset_counts(nrq_rxset *set, uint32_t *h_nlost, uint32_t *h_nrep);
/* nrq_rx_lists over all members, compact: h_nlost / h_nrep per block (nullable), and in h_lists (nullable, room for cap words)
 * block by block its repair ESIs in arrival order, then its missing source ESIs ascending -- word for word what nrq_rx_lists
 * gives for that member's block.  *h_total (nullable) = the words of all lists; cap < *h_total with h_lists given: -1, *h_total
 * and the counts still filled.  One listing pass on the device (a count per block, one scan, a fill per block), two downloads. */
int nrq_rxset_lists(nrq_rxset *set, uint32_t *h_nlost, uint32_t *h_nrep, uint32_t *h_lists, size_t cap, size_t *h_total);
/* nrq_rx_decode over all members: h_status[j] / h_used[j] (h_used nullable) per block, with nrq_rx_decode's meaning.  One listing
 * pass and one fetch for the whole set; the blocks nrq_rx_decode's rule selects -- gaps ng != 0, repair rows nr >= ng, nr - ng <=
 * max_esi - K; min(nr, ng + 2) repair symbols up front, the rest on demand -- grouped by (K, K', relay attached or not) across
 * the members, every group in calls of at most 256 blocks (the decode path's tested batch; a set holds 1024); ONE marking
 * launch.  A block without gaps has status 1 without work.
 * Afterwards every member is in the state its own nrq_rx_decode (nrq_orx_decode) would have left it in: the same verdict and
 * `used` per block, the same recovered source rows, the seen bits below K set and the gaps 0 of a recovered block (later packets
 * for it are IGN), repair rows and their ESI list untouched.  A member with a relay attached gets its recovered blocks'
 * intermediate symbols written into the relay's buffer, and those blocks are ready when the call returns, as documented for
 * nrq_rx_decode; members without one pass no intermediate address (the needed-pivot back-substitution stays).
 * An empty set, or nothing selectable: 0 and no decode launch (the listing pass still runs on a set with blocks).  h_status
 * NULL: -1 and an error text.  h_status is final on return; the solves and the marking are enqueued on the context's stream.
 * Errors: when a decode call fails, the blocks of the calls that succeeded before it are still marked -- their books say what
 * their rows hold -- the blocks of the failed and of the later calls have status 0 and their books as before, and the failing
 * call's code and text are returned.  A second nrq_rxset_decode finishes the job. */
int nrq_rxset_decode(nrq_rxset *set, int *h_status, uint32_t *h_used);
/* ---- what ALL members want or hold, with keys: the request of a whole set in one call ----
 * nrq_rxset_want / nrq_rxset_held: the list is the concatenation, in the set's block order (above), of what each member's own
 * nrq_rx_want / nrq_rx_held gives for the same arguments, word for word; d_keys[i] is the key of the member d_tags[i] belongs
 * to.  An attached object contributes what nrq_orx_want / nrq_orx_held gives (class L, then class S) under its one key.  Per block
 * the rules are the ones written at nrq_rx_want -- a complete block lists nothing, NRQ_WANT_SOURCE lists the clear source bits,
 * repair mode lists min(max(g + extra - r, 0), rep_cap - r) ESIs, the lowest unseen ones in [max(K, esi_from), max_esi] -- with
 * each MEMBER's own K, max_esi and rep_cap; the rank-deficiency note there applies as it stands.  Held lists a block's seen
 * source ESIs ascending, then its repair ESIs in arrival order, as nrq_rx_held.  (keys, tags) is the form nrq_txset_emit takes:
 * want -> emit -> nrq_rxset_add -> nrq_rxset_decode runs for all members without a per-member call or a host-built list.
 * The calling contract is nrq_rx_want's: the call waits for the work enqueued before it; *h_n, the total number of tags, is
 * final on return, and so is h_cnt (nullable): one entry per block in block order, as nrq_rxset_blocks reports them, the number
 * of tags that block lists, from the same download as the total.  d_tags NULL counts only; cap < *h_n: -1 with *h_n and h_cnt
 * still filled and nothing written; else the writing of d_tags and d_keys is enqueued on the context's stream, so an
 * nrq_txset_emit enqueued behind it sees both without a host wait (a read from the host or from another stream needs
 * nrq_ctx_sync first).  d_keys is nullable when d_tags is given (a set whose keys the caller does not need); d_keys without
 * d_tags: -1.  Argument errors are nrq_rx_want's; h_n NULL: -1.  An empty set: 0 with *h_n = 0 and no launch.  Three launches
 * (a count per block, one scan, a fill per block), one download and one wait for the whole set.  The call only reads the
 * members' books. */
int nrq_rxset_want(nrq_rxset *set, uint32_t flags, uint32_t extra, uint32_t esi_from, uint32_t *d_keys, uint32_t *d_tags, uint32_t cap,
                   uint32_t *h_cnt, uint32_t *h_n);
int nrq_rxset_held(nrq_rxset *set, uint32_t *d_keys, uint32_t *d_tags, uint32_t cap, uint32_t *h_cnt, uint32_t *h_n);

/* ---- sender sets: the packets of MANY transmissions and objects written into one buffer in one pass ----
 * The send-side counterpart of a reception set: a table of member transmissions (nrq_tx: senders and relays) and objects (nrq_otx:
 * object senders and objects' relays) of one context and one T, each under a 32-bit key.  nrq_txset_emit answers a request that
 * spans members -- packet k for (d_keys[k], d_tags[k]) -- with one chain of kernels, and with NRQ_TX_KEY_INLINE writes the packet
 * form nrq_rxset_add reads with NRQ_RX_KEY_INLINE, where today R members cost R emits into R buffers and a repack.  Members stay
 * ordinary transmissions: their own emit calls work between set calls.  The caps follow from the kernels: a linear search over
 * the table's segments per packet, one LDS counter and one ready bit per block. */
typedef struct nrq_txset nrq_txset;
#define NRQ_TXSET_MAX_SEGS   64u    /* table segments: a transmission is one, an object up to three */
#define NRQ_TXSET_MAX_BLOCKS 1024u  /* blocks over all members */
#define NRQ_TX_KEY_INLINE 4u        /* with NRQ_TX_TAG_INLINE: packet = key (32 bits, network byte order), FEC Payload ID, payload at +8 */
int nrq_txset_create(nrq_ctx *ctx, uint32_t T, nrq_txset **out);
void nrq_txset_destroy(nrq_txset *set); /* members live on, detached */
/* Attach a transmission, or an object (it owns its key), under `key`.  Refused (-1, nrq_ctx_error) by the rules of
 * nrq_rxset_attach: another context; a T that is not the set's; a transmission that is in a set already; a (key, SBN span) that
 * overlaps a member's; for an object, any other member under its key, and any further member under an object's key; a cap
 * exceeded.  Attach and detach wait for the context's stream (the table lives in device memory).  Destroying a member that is
 * still attached detaches it first. */
int nrq_txset_attach(nrq_txset *set, uint32_t key, nrq_tx *tx);
int nrq_txset_attach_obj(nrq_txset *set, uint32_t key, nrq_otx *tx);
int nrq_txset_detach(nrq_txset *set, uint32_t key); /* every member under key; unknown key: -1 */
/* The set's blocks in its block order -- members sorted by (key, first SBN), a member's blocks in SBN order -- as
 * nrq_rxset_blocks gives a reception set's.  Host state only. */
int nrq_txset_blocks(nrq_txset *set, uint32_t *h_keys, uint32_t *h_sbn, uint32_t cap, uint32_t *h_n);
/* Emit n packets (enqueue only, on the context's stream; no host wait): packet k at d_pkts + k*pkt_stride for key d_keys[k]
 * (device; NULL: every key is 0) and tag d_tags[k].  flags: NRQ_TX_TAG_INLINE, NRQ_TX_HELD, and with NRQ_TX_TAG_INLINE
 * NRQ_TX_KEY_INLINE (the key in front of the FEC Payload ID); pkt_stride >= T, + 4 with the tag inline, + 8 with key and tag.
 * A packet whose (key, SBN) names a member gets, byte for byte, the FEC Payload ID, the payload and the d_results entry (device,
 * nullable) that member's own nrq_tx_emit / nrq_otx_emit gives for that tag under the same NRQ_TX_TAG_INLINE and NRQ_TX_HELD
 * bits -- 0, or NRQ_TX_NOT_READY for a relay's block that is not ready, with the held-symbol table above under NRQ_TX_HELD.  The
 * members' ready state is taken as it is at this call.  NRQ_TX_HELD is accepted on any set: a member that is a plain sender has no
 * reception and answers as without the flag.  A packet that belongs to no member -- an unknown key, a key that is no object's
 * with an SBN outside its members, SBN >= Z of an object -- is left wholly untouched and gets -1.  n == 0 and an empty set: 0.
 * Refused (-1 and a text, nothing enqueued): NRQ_TX_KEY_INLINE without NRQ_TX_TAG_INLINE, an unknown flag, a stride too small,
 * NULL packets or tags, a member that is a sender and not encoded, a relay member whose reception was destroyed (the text names
 * the key). */
int nrq_txset_emit(nrq_txset *set, const uint32_t *d_keys, const uint32_t *d_tags, uint32_t n, void *d_pkts, size_t pkt_stride,
                   uint32_t flags, int32_t *d_results);

/* ---- sets: packets of several symbols ----
 * The set forms of nrq_rx_add_syms and nrq_tx_emit_syms: packets, keys and flags as in nrq_rxset_add / nrq_txset_emit; G, d_nsym
 * and the slot layout as in the several-symbol calls above, with hdr = 0, 4 (tag inline) or 8 (key and tag inline), symbol i at
 * hdr + i * T and pkt_stride >= hdr + G * T.  With NRQ_TX_KEY_INLINE / NRQ_RX_KEY_INLINE what the sender set writes is what the
 * reception set reads.  Both are enqueue-only on the context's stream.
 *
 * nrq_rxset_add_syms: every member ends with exactly what its own nrq_rx_add_syms (an attached object: nrq_orx_add_syms) gives
 * for the packets that carry its key, in packet order -- the same codes in the same slots of d_results (n * G entries, nullable),
 * the same rows, the same repair list in slot order, the same counts and seen bits.  With d_nsym NULL the count rule takes the K
 * of the member the first tag names.  A packet of an attached object's key with SBN >= Z gets what nrq_orx_add_syms gives it
 * (c slots ERR or IGN, c = d_nsym[k], or G without d_nsym; a count of 0 or above G: slot k * G ERR).  A packet of no member keeps
 * all its slots untouched and nothing of it is copied.  G = 1 with d_nsym NULL is nrq_rxset_add.  Refused: what nrq_rxset_add
 * refuses, G outside 1..NRQ_PKT_SYMS_MAX, a stride too small, n * G > 0x7FFFFFFF.
 *
 * nrq_txset_emit_syms: packet k is named by (d_keys[k], first tag d_tags[k], count).  A packet whose (key, SBN) names a member
 * gets, byte for byte, the header, the run of c_k payloads and the d_results[k] entry (n entries, nullable) that member's own
 * nrq_tx_emit_syms / nrq_otx_emit_syms gives: 0 written, NRQ_TX_NOT_READY a relay's block that is not ready, NRQ_TX_BAD_RANGE (a
 * sender is strict; the K of the member's segment decides the range); with NRQ_TX_KEY_INLINE the key goes in front of the FEC
 * Payload ID.  A packet of no member is wholly untouched and gets -1; the bytes behind hdr + c_k * T are untouched; no packet is
 * ever half written.  Ready bits are taken as they are at the call.  With NRQ_TX_HELD a member's packet gets what that member's
 * own call gives under the same bit (the table at nrq_tx_emit_syms): a ready block's packet is written as without the flag; one
 * of a block that is not ready, with an admissible range, is written iff the member's reception holds EVERY symbol e .. e+c-1 --
 * copies of the source rows, or of the repair rows found for the c ESIs -- else NRQ_TX_NOT_READY and untouched; an inadmissible
 * range is NRQ_TX_BAD_RANGE whether or not the block is ready; a member that is a plain sender answers as without the flag.
 * Refused: what nrq_txset_emit refuses, NRQ_TX_HELD on a set with NO relay member (the flag could do nothing there, as
 * nrq_tx_emit_syms refuses it on a sender; it is accepted as soon as one member is a relay or an object's relay; an EMPTY set has no relay member, so it refuses the flag
 * too, and so does a call with n = 0 on a set without one, although both return 0 at once without the flag), G outside
 * 1..NRQ_PKT_SYMS_MAX, a stride too small, n * G > 0x7FFFFFFF.
 *
 * nrq_rxset_want_syms / nrq_rxset_held_syms: the list is the concatenation, in the set's block order, of what each member's own
 * nrq_rx_want_syms / nrq_rx_held_syms (an attached object: nrq_orx_want_syms / nrq_orx_held_syms -- class L, then class S, each
 * with its own K, under the object's one key) gives for the same arguments, word for word: d_tags[k] a first tag, d_nsym[k] its
 * count, d_keys[k] the key of the member the packet belongs to.  Equivalently it is the packetisation (at nrq_rx_want_syms) of
 * nrq_rxset_want's / nrq_rxset_held's one-symbol list with each member's own K; its expansion is that list word for word, and
 * with G = 1 the first tags are that list and every count is 1.  (keys, tags, nsym) is the form nrq_txset_emit_syms takes: want
 * -> emit -> nrq_rxset_add_syms -> nrq_rxset_decode runs in packets for all members without a per-member call or a host-built
 * list.  The calling contract is nrq_rxset_want's and nrq_rx_want_syms' combined: the call waits for the work enqueued before it;
 * *h_npkt (required) is the number of packets, *h_nsym (nullable) the number of symbols -- the one-symbol call's *h_n -- and h_cnt
 * (nullable) one entry per block in block order, that block's number of PACKETS; all three are final on return and come from ONE
 * download and ONE wait.  d_tags and d_nsym both NULL: the counts only.  cap is in packets; cap < *h_npkt: -1 with the totals and
 * h_cnt still filled and nothing written; else the writing is enqueued on the context's stream, so an nrq_txset_emit_syms behind
 * it needs no host wait.  d_keys is nullable when the lists are given.  An empty set: 0 with zeros and no launch; a set that lists
 * nothing runs no fill launch.  Refused (-1 and a text, nothing enqueued): what nrq_rxset_want refuses, G outside
 * 1..NRQ_PKT_SYMS_MAX, exactly one of d_tags / d_nsym, d_keys without d_tags, h_npkt NULL.  The calls only read the members'
 * books. */
int nrq_rxset_want_syms(nrq_rxset *set, uint32_t flags, uint32_t extra, uint32_t esi_from, uint32_t G, uint32_t *d_keys, uint32_t *d_tags,
                        uint8_t *d_nsym, uint32_t cap, uint32_t *h_cnt, uint32_t *h_npkt, uint32_t *h_nsym);
int nrq_rxset_held_syms(nrq_rxset *set, uint32_t G, uint32_t *d_keys, uint32_t *d_tags, uint8_t *d_nsym, uint32_t cap, uint32_t *h_cnt,
                        uint32_t *h_npkt, uint32_t *h_nsym);
int nrq_rxset_add_syms(nrq_rxset *set, const void *d_pkts, size_t pkt_stride, const uint32_t *d_keys, const uint32_t *d_tags, uint32_t n,
                       uint32_t G, const uint8_t *d_nsym, uint32_t flags, int32_t *d_results);
int nrq_txset_emit_syms(nrq_txset *set, const uint32_t *d_keys, const uint32_t *d_tags, uint32_t n, uint32_t G, const uint8_t *d_nsym,
                        void *d_pkts, size_t pkt_stride, uint32_t flags, int32_t *d_results);

/* ---- sender sets: the range mode -- every member's symbols in one call, no list from the host ----
 * The carousel of a node that serves many objects or flows: the next symbols of every block of every member, fresh repair symbols
 * included, where nrq_txset_emit needs (d_keys[k], d_tags[k]) for every packet.  The set forms of nrq_tx_emit_range /
 * nrq_otx_emit_all and their _syms forms.
 *
 * The map.  The set's blocks are numbered g = 0 .. nb-1 in the set's block order (nrq_txset_blocks: members sorted by (key, first
 * SBN), a member's blocks in SBN order); block g has the K of its member (an object: of its block class).  A call names
 *   source (0 or 1): whether the block's K source symbols are sent;
 *   rep0, nrep:      the repair ESIs K + rep0 .. K + rep0 + nrep - 1 of every block, each block with its own K;
 *   G:               symbols per packet (1 in nrq_txset_emit_all).
 * Block g's packet list is the source run [0, K) cut into packets of G from its start, the last one short (only with source), then
 * the repair run [K + rep0, K + rep0 + nrep) cut the same way: len_g = (source ? ceil(K / G) : 0) + ceil(nrep / G) packets.  With
 * source = 1 and rep0 = 0 this is exactly the list of nrq_otx_emit_all_syms / nrq_tx_emit_range_syms(0, K + nrep), and
 * len_g = nrq_pkt_count(K, 0, K + nrep, G).  Packet j of block g has first tag (SBN_g << 24) | e, count c and key key_g.
 *   order 0 (block-major): packet (g, j) has index sum_{g' < g} len_g' + j.
 *   order 1 (interleaved): round j holds packet j of every block with len_g > j, in block order -- the rule nrq_otx_emit_all_syms
 *     states for order 1, over the set's block order; a block with fewer packets drops out of the later rounds.  The index of
 *     (g, j) is sum_{g'} min(len_g', j) + #{g' < g : len_g' > j}.
 *
 * nrq_txset_count_all: the packets of such a call, *h_npkt (nullable), and per block in block order h_cnt (nullable, room for
 * the set's blocks).  Host state only: no wait, no launch.  It refuses G, source and the totals as the emits do, and the ESI bound
 * with rep0 = 0.
 *
 * nrq_txset_emit_all_syms: packet k of the map at d_pkts + k*pkt_stride, byte for byte what nrq_txset_emit_syms writes for
 * (key_k, first tag_k, count_k) under the same flags -- one device pass computes the lists, then the list emit's own payload
 * kernels write the packets.  flags: NRQ_TX_TAG_INLINE, and with it NRQ_TX_KEY_INLINE; the header is 0, 4 or 8 bytes as in
 * nrq_txset_emit_syms, pkt_stride >= hdr + G * T, and the bytes behind hdr + c * T of a packet are untouched.  d_keys_out,
 * d_tags_out (n words each) and d_nsym_out (n bytes) receive the lists; each is nullable on its own (the lists then live in the
 * set's scratch).  *h_npkt (nullable) is the number of packets, final on return.  Enqueue only, on the context's stream, no host
 * wait; the members' ready state is taken as it is at the call.  nrq_txset_emit_all is nrq_txset_emit_all_syms with G = 1 and no
 * counts, through the one-symbol payload kernels of nrq_txset_emit.
 * An empty set, and source == 0 with nrep == 0: 0 with *h_npkt = 0 and no launch.
 * Refused (-1 and a text, nothing enqueued, nothing written): what nrq_txset_emit refuses -- a member that is not encoded, a relay
 * whose reception was destroyed, an unknown flag, NRQ_TX_KEY_INLINE without NRQ_TX_TAG_INLINE, NULL packets, a stride below
 * hdr + G * T; NRQ_TX_HELD (as nrq_tx_emit_range and nrq_otx_emit_all: every block is in the map); a relay member with a block that
 * is not ready (the text names the key and the first such SBN, as nrq_tx_emit_range on a relay); order or source outside {0, 1};
 * G outside 1..NRQ_PKT_SYMS_MAX; nrep > 0 with Kmax + rep0 + nrep - 1 > 0xFFFFFF (Kmax: the largest K in the set); more than
 * 0x7FFFFFFF packets, or packets * G above that -- found from the counts, before any allocation. */
int nrq_txset_count_all(nrq_txset *set, uint32_t source, uint32_t nrep, uint32_t G, uint32_t *h_cnt, uint32_t *h_npkt);
int nrq_txset_emit_all(nrq_txset *set, uint32_t source, uint32_t rep0, uint32_t nrep, int order, void *d_pkts, size_t pkt_stride,
                       uint32_t flags, uint32_t *d_keys_out, uint32_t *d_tags_out, uint32_t *h_npkt);
int nrq_txset_emit_all_syms(nrq_txset *set, uint32_t source, uint32_t rep0, uint32_t nrep, uint32_t G, int order, void *d_pkts,
                            size_t pkt_stride, uint32_t flags, uint32_t *d_keys_out, uint32_t *d_tags_out, uint8_t *d_nsym_out,
                            uint32_t *h_npkt);

/* Per-launch duration of the solve kernel, measured with HIP events recorded on the launch stream
 * immediately around each launch (bench.py's roofline leg).  enable(1) starts collecting; read()
 * synchronises, returns the durations of the launches since the last read/enable in launch order. */
int nrq_ktime_enable(nrq_ctx *ctx, int on);
int nrq_ktime_read(nrq_ctx *ctx, float *ms_out, uint32_t cap, uint32_t *count);
/* same for the decode planner (all kernels of a planner run, on the stream they run on) */
int nrq_ptime_read(nrq_ctx *ctx, float *ms_out, uint32_t cap, uint32_t *count);
/* same as intervals [start, start+dur) in ms after ref's nrq_ktime_enable(1); ref may be another context of the
 * same GPU, so that launches of several streams can be put on one time axis */
int nrq_ktime_read_intervals(nrq_ctx *ctx, nrq_ctx *ref, float *start_ms, float *dur_ms, uint32_t cap, uint32_t *count);

/* Generic stream timer (HIP events on the context's stream). */
int nrq_timer_start(nrq_ctx *ctx);
int nrq_timer_stop_ms(nrq_ctx *ctx, float *ms); /* synchronises */

#ifdef __cplusplus
}
#endif
#endif /* NANORQ_HIP_H */
