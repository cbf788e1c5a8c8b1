/*
 * lva_decoder.h -- C ABI of the MI355X list-Viterbi decoder (liblva_hip.so).
 *
 * Drop-in boundary for ONE path of shubhamchandak94/nanopore_dna_storage: the
 * convolutional-code parallel list-Viterbi decode of a flappie transition-posterior
 * matrix.  The reference has no library API for this path -- its boundary is the
 * subprocess `viterbi_nanopore.out -m decode -i X.post -o OUT ...` -- so each entry
 * point below cites the reference code it replaces
 * (file viterbi/viterbi_convolutional_code.cpp unless stated otherwise).
 *
 * Plain C types only: pointers, sizes, POD structs.  No torch / HIP types.
 * All functions return LVA_OK (0) or a negative LVA_ERR_* code; none aborts.
 */
#ifndef LVA_DECODER_H
#define LVA_DECODER_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LVA_OK 0
#define LVA_ERR_MEM_CONV (-1)        /* "Invalid mem_conv (allowed: 6, 8, 11, 14)"      :290-292 */
#define LVA_ERR_RATE (-2)            /* "Invalid rate parameter"                        :336-338 */
#define LVA_ERR_MSG_LEN (-3)         /* "Output length not even. Try padding ..."       :353-357 */
#define LVA_ERR_SYNC (-4)            /* sync marker too long / period short / bad char  :390-413 */
#define LVA_ERR_TOO_MANY_STATES (-5) /* runtime_error "Too many states"                 :595-597 */
#define LVA_ERR_POST_TOO_SHORT (-6)  /* runtime_error "Too small post matrix"           :600-601 */
#define LVA_ERR_MSG_TOO_LONG (-7)    /* runtime_error msg_len > BITSET_SIZE :604-605; uint8_t loop :831 */
#define LVA_ERR_NOMEM (-8)
#define LVA_ERR_HIP (-9)             /* a HIP runtime call failed (lva_last_hip_error has the text) */
#define LVA_ERR_ARG (-10)
#define LVA_ERR_NO_DEVICE (-11)      /* no gfx950 device visible: the product never falls back to CPU */
#define LVA_ERR_UNSUPPORTED (-12)
#define LVA_ERR_BUSY (-13)           /* lva_stream_submit: queue_cap reads already wait for a slot (back-pressure, nothing was taken);
                                        any batch entry point or a second lva_stream_open while the decoder has a stream open */

#define LVA_MAX_DEVIATION_DEFAULT 0xFFFFFFFFu /* reference default msg_len+mem_conv+1 (:238-240) */

typedef struct lva_decoder lva_decoder;

/* Decoder configuration = the decode-side CLI flags of the reference (:138-172):
 *   --mem-conv, -r/--rate, --msg-len, -l/--list-size, --max-deviation,
 *   --sync-marker, --sync-period.  (-t/--num-thr has no meaning on the GPU;
 *   --rc is per read, see lva_decode_batch.) */
typedef struct lva_config {
  int32_t mem_conv;
  int32_t rate;
  uint32_t msg_len;
  uint32_t list_size;
  uint32_t max_deviation;   /* LVA_MAX_DEVIATION_DEFAULT = unbanded */
  const char *sync_marker;  /* NULL or "" = none */
  uint32_t sync_period;
  int32_t device;           /* HIP device ordinal */
  int32_t max_slots;        /* reads in flight on the device; 0 = choose from free HBM */
  int32_t kernel;           /* 0 = default (4 where it is the faster one, else 2 where available, else 1); 1 = exact kernel,
                               one thread per target; 2 = fast kernel + exact fix-up (L = 1, 2, 4, 8: lva_step_fast /
                               lva_step_acs; any other 2 <= L <= 64: lva_step_big); 3 = exact kernel, one wavefront per
                               target (2 <= L <= 256: lva_step_wave up to 64 entries, lva_step_wave_wide above; never
                               the default); 4 = fast kernel with lazy messages (L = 2, 4, 8: messages materialised
                               every second time step, lva_step_lazy).  A mode whose kernels do not serve the list
                               size is LVA_ERR_UNSUPPORTED, any other value LVA_ERR_ARG; lva_kernel_plan tells what a
                               configuration resolves to.  Every mode gives the
                               reference's lists bit for bit on every input the reference decodes: targets the fast
                               kernels cannot decide (score ties, non-finite sums, fingerprint collisions) go through a
                               work list to an exact pass, and when that list overflows (tie-dense posteriors: quantised
                               or constant matrices) modes 2 and 4 redo the whole step on their exact path -- slower,
                               never refused (reference :762-796) */
  uint64_t mem_budget_bytes;/* cap on trellis memory; 0 = 60% of free HBM */
} lva_config;

/* Static facts about a code (set_conv_params :264-415). */
typedef struct lva_code_info {
  uint32_t nstate_pos, nstate_conv, oligo_len, msg_words;
  uint32_t initial_state, final_state;
  uint32_t g0, g1;
  int32_t pattern_len;
  uint8_t pattern[16];
} lva_code_info;

/* Counters of the last lva_decode_batch* call, or of the last stream after its close (bench.py's roofline object). */
typedef struct lva_profile {
  double step_kernel_ms;      /* HIP-event time from first to last trellis-step launch, on the decoder's stream */
  double total_ms;            /* HIP-event time of the whole call's device work (upload..results) */
  uint64_t step_launches;     /* trellis-step kernel launches */
  uint64_t read_steps;        /* sum over reads of nblk (one launch advances every active read one step) */
  double algorithmic_bytes;   /* sum over reads of sum_t [2 R(t) L (4+4W) + 160] */
  uint64_t fixup_states;      /* states redone by the exact kernel (kernel mode 2); a launch whose work list overflowed
                                 counts in overflow_steps instead (every state of the step was redone) */
  uint64_t fixup_reason[4];   /* of which: score tie on top, non-finite arithmetic, too many fingerprint
                                 matches, fingerprint collision */
  int32_t slots;              /* reads in flight */
  int32_t kernel;             /* kernel mode used */
  /* with lva_decoder_set_launch_events(d, 1): HIP events around every trellis-step launch */
  double dominant_kernel_ms;  /* sum over launches of the dominant kernel alone (lva_step_fast / lva_step_big / ...) */
  double step_pair_ms;        /* sum over launches of dominant kernel + fix-up pass */
  uint64_t timed_launches;    /* launches in those sums */
  double h2d_ms;              /* lva_decode_batch: HIP-event time of the host->device copy of the posteriors */
  uint64_t h2d_bytes;
  uint64_t overflow_steps;    /* launches whose work list of undecided targets overflowed: the exact path redid the whole
                                 step (tie-dense posteriors; correct, but a large slow-down the caller can now see) */
  double working_bytes;       /* algorithmic_bytes' sum over the band the kernels actually work on (lva_band_table's
                                 working_lo_hi): the bytes that are moved, about 5 % fewer at the benchmark shape */
} lva_profile;

/* "lva_hip <abi>.<n> (gfx950) build <id>": <id> is a hash of the library's source files taken when it was built
 * (csrc/Makefile), so that a profile or a counter file can name the library it was measured on (bench.py writes it into
 * every JSON line; profiles/ *_traffic.json carry it). */
const char *lva_version(void);
/* LVA_ABI_VERSION of the library that was loaded.  It changes whenever a struct of this header changes size or layout
 * (5: lva_profile gained overflow_steps and working_bytes): a caller built against another value must not pass structs.
 * Entry points added since (lva_stream_*, lva_transpost_*, lva_device_download, lva_list_*, lva_demux_*, lva_kernel_plan,
 * lva_align_profile, lva_map_index_*, lva_map_reads, lva_map_reads_pooled, lva_score_bases*, lva_trace_bases*,
 * lva_forward_bases*) change no struct and keep it at 5. */
#define LVA_ABI_VERSION 5
int lva_abi_version(void);
const char *lva_strerror(int code);
const char *lva_last_hip_error(void);

/* --- host-only: code parameters and the encoder ------------------------------------------- */

/* set_conv_params (:264-415): validate and describe a code. */
int lva_code_describe(int32_t mem_conv, int32_t rate, uint32_t msg_len, int32_t rc,
                      const char *sync_marker, uint32_t sync_period, lva_code_info *out);

/* The tables the kernels use, for inspection/tests.  Each output may be NULL.
 *   pos2msg[nstate_pos], ptype[nstate_pos], vmask[nstate_pos], vval[nstate_pos],
 *   predtab[4][nstate_conv] (uint16, zero rows for unused block types). */
int lva_code_tables(int32_t mem_conv, int32_t rate, uint32_t msg_len, int32_t rc,
                    const char *sync_marker, uint32_t sync_period, uint32_t *pos2msg, uint8_t *ptype,
                    uint32_t *vmask, uint32_t *vval, uint16_t *predtab);

/* The 32-bit message fingerprint the step kernels hold for a path that has consumed n_bits <= msg_len message bits (the
 * de-duplication key of the fast kernels), for inspection/tests: the kernels' per-position
 * deltas folded from the empty message.  msg_bits: msg_len bytes of 0/1 in lva_encode's order; the forward orientation
 * consumes msg_bits[0 .. n_bits), a reverse complement (rc != 0) msg_bits[msg_len - 1] down to msg_bits[msg_len - n_bits].
 * n_bits = msg_len goes on through the terminating bits: the fingerprint at the final position.  LVA_ERR_ARG when
 * n_bits > msg_len or when no trellis position has consumed exactly n_bits bits (inside a two-bit position). */
int lva_code_fingerprint(int32_t mem_conv, int32_t rate, uint32_t msg_len, int32_t rc, const char *sync_marker,
                         uint32_t sync_period, const uint8_t *msg_bits, uint32_t n_bits, uint32_t *out);

/* The band [lo, hi) of every time step of a read of nblk blocks, for inspection/tests (each output may be NULL, 2*nblk words):
 *   reference_lo_hi  as the reference computes it (:677-679, with the fused multiply-subtract of its build);
 *   working_lo_hi    what the kernels work on: the same without positions a path cannot have reached yet (> t + 1) and
 *                    positions that cannot reach the final one any more (< nstate_pos - nblk + t) -- their lists never
 *                    reach the output, so they are neither written nor read. */
int lva_band_table(int32_t mem_conv, int32_t rate, uint32_t msg_len, int32_t rc, const char *sync_marker,
                   uint32_t sync_period, uint32_t nblk, uint32_t max_deviation, uint32_t *reference_lo_hi,
                   uint32_t *working_lo_hi);

/* `-m encode` (:215-225): conv_encode (:450-499) + 2-bit base packing (:540-551).
 * msgs: n_msgs*msg_len bytes of 0/1.  out_bases: n_msgs*oligo_len bytes, values 0..3 = A,C,G,T. */
int lva_encode(int32_t mem_conv, int32_t rate, uint32_t msg_len, const uint8_t *msgs, int32_t n_msgs,
               uint8_t *out_bases);

/* SURVEY 8(d) algorithmic bytes of one read of nblk blocks. */
int lva_algorithmic_bytes(int32_t mem_conv, int32_t rate, uint32_t msg_len, int32_t rc,
                          const char *sync_marker, uint32_t sync_period, uint32_t nblk,
                          uint32_t list_size, uint32_t max_deviation, double *out);

/* Which step kernel a configuration runs, and on which trellis layout: what lva_decoder_create decides before it looks at a
 * device (csrc/lva_plan.h plan_kernels; the table is in DESIGN.md section 4). */
#define LVA_STEP_EXACT 0      /* lva_step_exact */
#define LVA_STEP_WAVE 1       /* lva_step_wave */
#define LVA_STEP_WAVE_WIDE 2  /* lva_step_wave_wide<instance>, instance = ceil(list_size / 64) */
#define LVA_STEP_ACS 3        /* lva_step_acs */
#define LVA_STEP_FAST 4       /* lva_step_fast */
#define LVA_STEP_LAZY 5       /* lva_step_lazy */
#define LVA_STEP_BIG 6        /* lva_step_big<instance>, instance = 16, 32 or 64 list entries */
#define LVA_STEP_BIG_REC 7    /* lva_step_big_rec<instance>, instance = 32 or 64 */
#define LVA_FIXUP_NONE 0
#define LVA_FIXUP_WAVE 1      /* lva_step_fixup_wave */
#define LVA_FIXUP_LAZY 2      /* lva_step_fixup_lazy */
typedef struct lva_kernel_plan_info {
  int32_t mode;             /* the kernel mode that runs, 1..4: lva_profile.kernel of a decoder of this configuration */
  int32_t dominant;         /* LVA_STEP_* */
  int32_t fixup;            /* LVA_FIXUP_*: the exact pass over the dominant kernel's work list */
  uint32_t lazy, rec, cmp;  /* layout: back-pointer bytes behind every list, record layout, compact lists at one-bit positions */
  uint32_t ring_positions;  /* trellis positions stored per parity buffer */
  int32_t instance;         /* template instance of the dominant kernel where it has one (above), else 0 */
} lva_kernel_plan_info;

/* Host only, opens no device.  Its refusals are lva_decoder_create's first ones, in the same order: LVA_ERR_ARG for a list_size
 * outside 1..65535, the code's errors, LVA_ERR_MSG_TOO_LONG, LVA_ERR_TOO_MANY_STATES for the state index, LVA_ERR_ARG for a
 * kernel outside 0..4, LVA_ERR_UNSUPPORTED for a kernel mode that does not serve the list size.  (lva_decoder_create then lays
 * the trellis out -- LVA_ERR_TOO_MANY_STATES when one parity buffer passes 2^32 words -- and only then looks at the device.)
 * cfg->device, max_slots and mem_budget_bytes are not looked at. */
int lva_kernel_plan(const lva_config *cfg, lva_kernel_plan_info *out);

/* --- decoder ------------------------------------------------------------------------------ */

/* Replaces process start-up of `viterbi_nanopore.out -m decode` (main :137-214, set_conv_params,
 * table construction :624-650).  The configuration is checked first (lva_kernel_plan's errors), then the device:
 * LVA_ERR_NO_DEVICE when no GPU is usable. */
int lva_decoder_create(const lva_config *cfg, lva_decoder **out);
void lva_decoder_destroy(lva_decoder *d);

/* Replaces read_crf_post (:553-575) + decode_post_conv_parallel_LVA (:589-858) + the list
 * writer (:248-253) for n_reads independent reads.
 *   post         host float32, all reads' .post matrices back to back, 40 floats per block
 *                (file order: rows 0-3 = into flip base b from state s at [b*8+s], row 4 = into flop);
 *   row_offsets  n_reads+1 block offsets into post (read i = blocks [off[i], off[i+1]));
 *   rc_flags     n_reads bytes, 1 = decode as reverse complement (--rc), NULL = all forward;
 *   out_msgs     n_reads*list_size*msg_len bytes of 0/1, best first (rows >= count untouched);
 *   out_scores   n_reads*list_size path scores (may be NULL);
 *   out_counts   n_reads: number of list entries (<= list_size), or a negative LVA_ERR_* for a
 *                read the reference would have thrown on (e.g. LVA_ERR_POST_TOO_SHORT). */
int lva_decode_batch(lva_decoder *d, const float *post, const int64_t *row_offsets, int32_t n_reads,
                     const uint8_t *rc_flags, uint8_t *out_msgs, float *out_scores, int32_t *out_counts);

/* Same, with `post` already resident in device memory (HBM) of the decoder's device. */
int lva_decode_batch_device(lva_decoder *d, const float *post_dev, const int64_t *row_offsets,
                            int32_t n_reads, const uint8_t *rc_flags, uint8_t *out_msgs,
                            float *out_scores, int32_t *out_counts);

/* As lva_decode_batch_device, but read i is the window of n_blocks[i] blocks that starts at block
 * first_block[i] of the resident buffer: decodes the payload windows found by
 * lva_locate_payload_batch_device in place.
 * replaces: helper.truncate_post_file (helper.py:212-224) + the decode call of generate_decoded_lists.py:80-89. */
int lva_decode_windows_device(lva_decoder *d, const float *post_dev, const int64_t *first_block, const int64_t *n_blocks,
                              int32_t n_reads, const uint8_t *rc_flags, uint8_t *out_msgs, float *out_scores,
                              int32_t *out_counts);

int lva_decoder_profile(const lva_decoder *d, lva_profile *out);
/* on != 0: record HIP events around every trellis-step launch of later decode calls (three per launch, on the
 * decoder's stream) so that lva_profile carries per-kernel times measured live; off by default. */
int lva_decoder_set_launch_events(lva_decoder *d, int32_t on);

/* --- decode stream ------------------------------------------------------------------------
 * A decoder that stays resident and is fed while it runs: reads go in one at a time, launches are shared by whatever is
 * in flight, results come out as they finish.  A read's list and scores are those of lva_decode_batch, bit for bit,
 * whenever it was submitted and whatever else is in flight.  The library starts no thread: lva_stream_poll drives the
 * stream.  One stream per decoder; while it is open every batch entry point of that decoder (lva_decode_*, lva_basecall_*,
 * lva_locate_payload_*, lva_find_barcode_batch, lva_demux_*) returns LVA_ERR_BUSY.
 * replaces: the process per read of helper.py:305, simulator.py:85 and generate_decoded_lists.py:90, and the side-by-side
 * driver copies the reference scales with (util/extra/generate_read_id_files.py:23-36, merge_lists.py:11-21). */
typedef struct lva_stream lva_stream;

/* queue_cap >= 1: reads that may wait for a slot.  Resets the decoder's profile counters. */
int lva_stream_open(lva_decoder *d, int32_t queue_cap, lva_stream **out);
/* Waits for what is enqueued on the device, drops reads that have not been handed out, frees the stream.  The decoder takes
 * batch calls again; lva_decoder_profile then reports the stream's totals (launches, read-steps, algorithmic and working
 * bytes, fix-up counters, overflow steps, event times from open to close; the per-launch event sums stay zero). */
int lva_stream_close(lva_stream *s);
/* One read: read_crf_post (:553-575) of a host float32 [n_blocks][40] matrix, copied before the call returns.  Never waits
 * for a decode.  LVA_ERR_BUSY when queue_cap reads already wait for a slot (nothing taken: poll, then submit again).  A read
 * the reference would refuse (n_blocks < nstate_pos + 1, :600-601) is accepted and comes back from lva_stream_poll with
 * count LVA_ERR_POST_TOO_SHORT.  rc != 0: decode as reverse complement (--rc).  tag: the caller's name of the read. */
int lva_stream_submit(lva_stream *s, const float *post, int64_t n_blocks, int32_t rc, uint64_t tag);
/* decode_post_conv_parallel_LVA (:589-858) + the list writer (:248-253), a step at a time: enqueues launch groups while a
 * slot is active (at most 32 launches ahead of the device), refills free slots from the queue in submission order, and hands
 * out up to max_reads finished reads in the order they finished, in the layout of lva_decode_batch:
 *   tags[k], out_msgs[k][list_size][msg_len] (rows >= count untouched), out_scores[k][list_size] (may be NULL),
 *   out_counts[k] (entries, or a negative LVA_ERR_*); *n_out reads were written.
 * wait = 0 never blocks on the device; wait = 1 returns as soon as at least one read is finished or nothing is pending. */
int lva_stream_poll(lva_stream *s, int32_t wait, int32_t max_reads, uint64_t *tags, uint8_t *out_msgs, float *out_scores,
                    int32_t *out_counts, int32_t *n_out);
/* queued: waiting for a slot; in_slots: in a slot, or out of it with the result still on its way to the host;
 * finished: ready for lva_stream_poll.  Each may be NULL. */
int lva_stream_pending(const lva_stream *s, int32_t *queued, int32_t *in_slots, int32_t *finished);

/* Device helpers so that callers without a HIP binding (ctypes) can keep inputs resident. */
int lva_device_alloc(lva_decoder *d, uint64_t bytes, void **out_dev_ptr);
int lva_device_free(lva_decoder *d, void *dev_ptr);
int lva_device_upload(lva_decoder *d, void *dev_dst, const void *host_src, uint64_t bytes);
int lva_device_synchronize(lva_decoder *d);
/* The counterpart of lva_device_upload: device -> host on the decoder's stream, complete on return. */
int lva_device_download(lva_decoder *d, void *host_dst, const void *dev_src, uint64_t bytes);

/* ---------------------------------------------------------------------------------------------
 * transition posteriors of a flip-flop CRF from the network's raw transition
 * scores, so that the chain on the device starts where a network ends:
 * scores -> posteriors -> basecall -> barcode -> window -> lists.
 * scores: float32 [blocks][40] per read, reads back to back with row_offsets[n_reads+1] as for lva_decode_batch
 * (row_offsets[0] = 0), in the layout of flappie's `trans` matrix and of .post: [b*8+s] = score of entering
 * flip base b from state s, [32+s] = score of entering flop (from flip s for s < 4, staying in flop s otherwise).
 * The output has the same shape and holds log-posteriors: the log-sum-exp of every block is 0.  Forward and
 * backward vectors start at 0 for all 8 states (decode.c:386, :425).  fp32, in an order of the library's own (the
 * values agree with a float64 forward-backward to a few 1e-6; flappie's own float32 chain is further from it).
 * Non-finite scores give what IEEE arithmetic gives for that read; other reads are unaffected.  A read may have
 * no block.  Limits as for the basecall entry points below: 2^20 blocks per read, fewer than 2^31 per batch,
 * otherwise LVA_ERR_ARG (decided from the offsets, before anything is allocated).  Device buffers are 16-byte
 * aligned.  Both calls run on the decoder's stream and are complete on return; LVA_ERR_BUSY while a decode stream
 * is open.  Afterwards lva_decoder_profile reports total_ms = HIP-event time of the two kernels and read_steps =
 * blocks of the batch (slots and kernel as before, everything else 0).
 * ------------------------------------------------------------------------------------------- */

/* replaces: transpost_crf_flipflop(trans, true) (flappie/src/decode.c:377-497) + log_row_normalise_inplace
 * (flappie/src/flappie_matrix.c:450-467) */
int lva_transpost_batch(lva_decoder *d, const float *scores, const int64_t *row_offsets, int32_t n_reads, float *post_out);
/* Same with the scores resident on the decoder's device.  post_dev may equal scores_dev (in place); otherwise the two
 * must not overlap.  The result is what lva_basecall_batch_device, lva_locate_payload_batch_device,
 * lva_decode_batch_device and lva_decode_windows_device take: no copy in between. */
int lva_transpost_batch_device(lva_decoder *d, const float *scores_dev, const int64_t *row_offsets, int32_t n_reads,
                               float *post_dev /* may equal scores_dev */);

/* ---------------------------------------------------------------------------------------------
 * the step in front of the list decoder on real data -- flappie's
 * flip-flop basecall of the posterior matrix and the barcode localisation on it, so that the
 * whole .post -> payload window -> decoded list chain stays on the device.
 * Posterior matrices are passed as for lva_decode_batch: one float32[blocks][40] buffer and
 * row_offsets[n_reads+1] in blocks (row_offsets[0] = 0).  A read may have at most 2^20 blocks (or called
 * bases) and a batch fewer than 2^31 blocks in all; beyond that the calls return LVA_ERR_ARG.
 * ------------------------------------------------------------------------------------------- */

/* Result of a barcode search for one read.
 * replaces: the tuple returned by helper.find_barcode_pos_in_post (helper.py:157-210) and the
 * orientation / length decision of generate_decoded_lists.py:68-79. */
typedef struct lva_payload_pos {
  int32_t start_pos, end_pos;   /* payload = blocks [start_pos, end_pos] of the read's matrix; -1, -1 on failure */
  int32_t dist_start, dist_end; /* edit distance of the best start / end barcode match; INT32_MAX = the reference's np.inf */
  int32_t rc;                   /* 1: the reverse-complement barcodes matched better (generate_decoded_lists.py:71-74) */
  int32_t ok;                   /* 0: "Failure in barcode removing." (generate_decoded_lists.py:76) */
} lva_payload_pos;

/* Basecall: the base string flappie writes as the second fastq line and the positions it writes
 * to --trans-output-file.
 * replaces: decode_crf_flipflop (flappie/src/decode.c:119-204), change_positions (decode.c:66-79)
 * and the loop of flappie/src/flappie.c:274-285.
 * Outputs of read i start at row_offsets[i] in bases_out / trans_out (capacity row_offsets[n_reads]
 * each; either may be NULL); nbases_out[i] = number of bases called. */
int lva_basecall_batch(lva_decoder *d, const float *post, const int64_t *row_offsets, int32_t n_reads,
                       char *bases_out, uint32_t *trans_out, int32_t *nbases_out);
int lva_basecall_batch_device(lva_decoder *d, const float *post_dev, const int64_t *row_offsets, int32_t n_reads,
                              char *bases_out, uint32_t *trans_out, int32_t *nbases_out);

/* Barcode search on given basecalls (one orientation).
 * replaces: helper.find_barcode_pos_in_post (helper.py:157-210); rc = 0, ok = (start_pos != -1).
 * bases / trans hold the basecall and the trans-file integers of read i at
 * [base_offsets[i], base_offsets[i+1]).  Barcodes: 1..64 characters. */
int lva_find_barcode_batch(lva_decoder *d, const char *bases, const uint32_t *trans, const int64_t *base_offsets,
                           int32_t n_reads, const char *start_barcode, const char *end_barcode, lva_payload_pos *out);

/* Basecall + barcode search in both orientations + the choice between them.
 * replaces: generate_decoded_lists.py:68-79 (START_BARCODE_RC = rc(end), END_BARCODE_RC = rc(start), :33-34);
 * min_len = MEM_CONV + MSG_LEN + 1 (:76).  The caller then decodes blocks [start_pos, end_pos]
 * with the rc flag (lva_decode_windows_device on the same resident buffer: no copy). */
int lva_locate_payload_batch(lva_decoder *d, const float *post, const int64_t *row_offsets, int32_t n_reads,
                             const char *start_barcode, const char *end_barcode, uint32_t min_len, lva_payload_pos *out);
int lva_locate_payload_batch_device(lva_decoder *d, const float *post_dev, const int64_t *row_offsets, int32_t n_reads,
                                    const char *start_barcode, const char *end_barcode, uint32_t min_len,
                                    lva_payload_pos *out);

/* ---------------------------------------------------------------------------------------------
 * DESIGN.md section 1 row N3': demultiplexing a pooled run.  The reference's real data is ONE sequencing run of
 * thirteen experiments, each with its own barcode pair and its own code (the table of encode_experiments.py:3-33, used at
 * :117-128); it sorts the pooled reads with an aligner (util/align_compute_stats.sh + util/generate_read_id_file.py) and
 * then runs generate_decoded_lists.py:68-79 once per experiment.  Here a read is basecalled once, its basecall is searched
 * for every experiment's barcodes in one launch, and one decision per read names the experiment, the orientation and the
 * payload window; the caller decodes each group with its own code from the same resident buffer
 * (lva_decode_windows_device).
 *
 * For every experiment e the candidate is what lva_locate_payload_batch gives for (start_barcode, end_barcode, min_len) of
 * exps[e].  A candidate is located when start_pos != -1; its total is dist_start + dist_end.  The located candidate with the
 * smallest total wins (the lowest e on a draw); the runner-up is the located candidate with the smallest total among the
 * OTHER experiments (runner_up = -1, runner_up_dist = INT32_MAX when there is none).  reason is the first that applies:
 *   1  no candidate is located            (experiment = -1, pos = {-1, -1, INT32_MAX, INT32_MAX, 0, 0})
 *   2  max_dist >= 0 and total > max_dist
 *   3  runner_up_dist - total < min_margin (a missing runner-up never is too close)
 *   4  the winner's window is shorter than its min_len (the candidate's ok is 0)
 *   0  none: the read is assigned
 * and in cases 0, 2, 3, 4 pos is the winner's candidate with ok = (reason == 0).
 * 1 <= n_exps <= 64; barcodes of 1..64 characters out of ACGTN (an N, in a barcode or in a basecall, matches nothing);
 * min_margin >= 0; otherwise LVA_ERR_ARG before the device is touched.  n_reads = 0 succeeds and touches nothing.  Read
 * limits, LVA_ERR_BUSY and "complete on return" as for lva_locate_payload_batch.
 * ------------------------------------------------------------------------------------------- */
typedef struct lva_experiment_barcodes {
  const char *start_barcode, *end_barcode;
  uint32_t min_len;             /* MEM_CONV + MSG_LEN + 1 of the experiment's code (generate_decoded_lists.py:76) */
} lva_experiment_barcodes;

typedef struct lva_demux_pos {
  lva_payload_pos pos;
  int32_t experiment;           /* the winner, -1 when nothing is located */
  int32_t reason;               /* 0: assigned; 1..4 above */
  int32_t runner_up, runner_up_dist;
} lva_demux_pos;

/* replaces: util/align_compute_stats.sh + util/generate_read_id_file.py (the reference's sorting step) and
 * generate_decoded_lists.py:68-79 per experiment of encode_experiments.py:3-33.
 * all_out: [n_reads][n_exps] candidates, may be NULL. */
int lva_demux_batch(lva_decoder *d, const float *post, const int64_t *row_offsets, int32_t n_reads,
                    const lva_experiment_barcodes *exps, int32_t n_exps, int32_t max_dist /* < 0: none */,
                    int32_t min_margin, lva_demux_pos *out, lva_payload_pos *all_out);
/* Same with the posteriors resident on the decoder's device (lva_device_alloc / lva_transpost_batch_device). */
int lva_demux_batch_device(lva_decoder *d, const float *post_dev, const int64_t *row_offsets, int32_t n_reads,
                           const lva_experiment_barcodes *exps, int32_t n_exps, int32_t max_dist, int32_t min_margin,
                           lva_demux_pos *out, lva_payload_pos *all_out);
/* Same on given basecalls (bases / trans / base_offsets as for lva_find_barcode_batch), both orientations.
 * replaces: helper.find_barcode_pos_in_post (helper.py:157-210) twice per experiment + generate_decoded_lists.py:68-79. */
int lva_demux_bases_batch(lva_decoder *d, const char *bases, const uint32_t *trans, const int64_t *base_offsets,
                          int32_t n_reads, const lva_experiment_barcodes *exps, int32_t n_exps, int32_t max_dist,
                          int32_t min_margin, lva_demux_pos *out, lva_payload_pos *all_out);

/* ---------------------------------------------------------------------------------------------
 * the Reed-Solomon outer code, RS(65535, 65535 - redundancy) over GF(2^16)
 * (primitive polynomial x^16+x^12+x^3+x+1, generator roots alpha^0 .. alpha^(redundancy-1)) shortened to n_total
 * symbols -- one codeword per 16-bit column of the oligo payloads, all columns in one call.
 * Symbols are uint16 in host byte order = the little-endian 2-byte pieces the reference reads from its files
 * (RSCode_schifra/schifra_RS_16bit_fileio.cpp:89-103).  1 <= redundancy <= 4096, redundancy < n_total <= 65535.
 * pad_symbol = the value of the 65535 - n_total untransmitted leading symbols (the reference pads with ASCII '0'
 * bytes: 0x3030, RSCode_16bit_fileio.py:58,:104).
 * ------------------------------------------------------------------------------------------- */

/* replaces: RS_decode_16bit for every column (RSCode_schifra/RSCode_16bit_fileio.py:87-137) =
 * schifra decoder::decode(block, erasure_list) (RSCode_schifra/schifra_reed_solomon_decoder.hpp:64-168).
 *   symbols   [n_codewords][n_total] received words (the reference puts pad_symbol at erased positions, :242-250);
 *   erasures  n_erasures distinct positions in [0, n_total), shared by all codewords;
 *   out       [n_codewords][n_total - redundancy] decoded data symbols; where the reference's decoder gives up
 *             (no output file, :122-123) every symbol is fail_symbol (the reference: ASCII '0' bytes, 0x3030);
 *   ok        [n_codewords] 1 = decoded, 0 = given up (may be NULL). */
int lva_rs_decode(int32_t device, const uint16_t *symbols, int32_t n_codewords, int32_t n_total, int32_t redundancy,
                  const int32_t *erasures, int32_t n_erasures, uint16_t pad_symbol, uint16_t fail_symbol, uint16_t *out,
                  int32_t *ok);

/* replaces: RS_encode_16bit for every column (RSCode_16bit_fileio.py:48-77) = schifra encoder::encode
 * (schifra_reed_solomon_encoder.hpp:57-88): systematic; out [n_codewords][n_data + redundancy] = data, then parity. */
int lva_rs_encode(int32_t device, const uint16_t *data, int32_t n_codewords, int32_t n_data, int32_t redundancy,
                  uint16_t pad_symbol, uint16_t *out);
const char *lva_rs_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * what happens to a decoded list -- the step between lva_decode_batch and
 * lva_rs_decode.  Inputs are the decoder's own outputs, as they are:
 *   msgs    uint8 [n_reads][list_size][msg_len] of 0/1, best first (only bit 0 of a byte is looked at);
 *   counts  int32 [n_reads]; a count <= 0 (a negative LVA_ERR_* included) means "no list", a count above list_size
 *           counts as list_size.
 * 1 <= msg_len <= 255, list_size >= 1, n_reads * list_size * msg_len < 2^31; n_reads = 0 succeeds and touches nothing.
 * Like lva_rs_decode the calls take a device ordinal, not a decoder: they work on a stream of their own, are complete
 * on return and leave every lva_profile alone.  All results are integers and exact; the same inputs give the same
 * bytes on every run.  Arguments are checked before the device is touched (LVA_ERR_ARG); without a gfx950 device
 * the calls return LVA_ERR_NO_DEVICE (no CPU path); a HIP failure is LVA_ERR_HIP with the text in lva_last_hip_error.
 * ------------------------------------------------------------------------------------------- */

/* replaces: helper.decode_list_CRC_index (helper.py:371-388) for every read of a batch.
 * Of read i the first min(counts[i], use_entries) entries are tried in order (use_entries = 0: list_size; the
 * `[:list_size]` slices of compute_error_rate_from_decoded_lists.py:37 and decode_RS_from_decoded_lists.py:41).  An entry
 * is accepted when -- without its last bit if pad -- the CRC-8 (polynomial 0x07, start 0, not reflected, no final xor)
 * of all its bytes but the last equals the last byte, and its first 12 bits x give an index
 * 3303 * (x - 2532) mod 4096 (helper.py:28-32) below num_oligos.  msg_len must be 12 + 8 * bytes_per_oligo + 8 + (pad ? 1 : 0),
 * the one shape helper.compute_parameters (helper.py:352-363) produces; 1 <= num_oligos <= 4096.
 *   out_index   [n_reads] index of the accepted entry, -1: none;
 *   out_rank    [n_reads] its place in the list, -1: none;
 *   out_payload [n_reads][bytes_per_oligo] its payload, zeros: none. */
int lva_list_filter(int32_t device, const uint8_t *msgs, const int32_t *counts, int32_t n_reads, int32_t list_size,
                    uint32_t msg_len, int32_t use_entries /* 0 = list_size */, int32_t bytes_per_oligo, int32_t num_oligos,
                    int32_t pad, int32_t *out_index, int32_t *out_rank, uint8_t *out_payload);

/* replaces: the per-index vote of decode_RS_from_decoded_lists.py:37-51 over lva_list_filter's outputs; with first_only
 * the rule of helper.simulate_and_decode instead (helper.py:326-329: the first payload seen for an index stands).
 *   index [n_reads], payload [n_reads][bytes_per_oligo] in read order; a negative index is a read without a vote,
 *   an index >= num_oligos is LVA_ERR_ARG.  1 <= num_oligos <= 4096, n_reads * bytes_per_oligo < 2^31.
 * Per index the payload with the most votes wins, among equal counts the one that reached that count first in read
 * order (what the reference's stable re-sort after every read gives).
 *   out_present [num_oligos] 1: some read voted for the index;
 *   out_payload [num_oligos][bytes_per_oligo] the winner, zeros where absent;
 *   out_votes   [num_oligos] reads that carried the winner, 0 where absent.
 * The rows with out_present = 1 are lva_rs_decode's received reads, the others its erasures. */
int lva_list_consensus(int32_t device, const int32_t *index, const uint8_t *payload, int32_t n_reads, int32_t bytes_per_oligo,
                       int32_t num_oligos, int32_t first_only, uint8_t *out_present, uint8_t *out_payload, int32_t *out_votes);

/* Per-read statistics of a decoded list against the message that was sent.
 * replaces: the per-trial part of simulator.py:92-110 (distance.hamming, distance.levenshtein, the 8- and 16-bit block
 * comparisons).  All fields are -1 for a read without a list. */
typedef struct lva_list_stat {
  int32_t top_correct;  /* the first entry equals the truth */
  int32_t list_correct; /* one of the counts[i] entries does */
  int32_t hamming;      /* differing bits of the first entry */
  int32_t hamming8;     /* differing blocks of 8 bits (the last block may be short) */
  int32_t hamming16;    /* differing blocks of 16 bits */
  int32_t edit;         /* unit-cost Levenshtein distance between truth and first entry */
} lva_list_stat;
/* truth: uint8 [n_reads][msg_len] of 0/1; out [n_reads]. */
int lva_list_stats(int32_t device, const uint8_t *msgs, const int32_t *counts, const uint8_t *truth, int32_t n_reads,
                   int32_t list_size, uint32_t msg_len, lva_list_stat *out);

/* ---------------------------------------------------------------------------------------------
 * DESIGN.md section 1 row N4': reading-cost trials -- the loop of decode_RS_from_decoded_lists.py:30-66 (draw a sample of
 * the reads, vote per index, RS-decode, compare with the original file) for n_trials trials and n_points sample sizes
 * in one call.  Which reads trial t draws, and in which order, is defined by a keyed permutation of the read numbers
 * (nanopore_dna_storage_amd/trials.py: Feistel network over Philox4x32-10, stream 5, with cycle walking; the sample of size
 * u is its first u reads, so the samples of one trial are nested); a trial depends on (seed, trial number) alone.
 *   index [n_reads], payload [n_reads][bytes_per_oligo]: lva_list_filter's outputs for ALL read numbers (a read without a
 *                  list: index -1); an index >= num_oligos is LVA_ERR_ARG;
 *   bytes_per_oligo even and >= 2; 1 <= num_oligos <= 4096; 1 <= redundancy <= min(4096, num_oligos - 1);
 *   original       the file, 1 <= original_bytes <= (num_oligos - redundancy) * bytes_per_oligo;
 *   reads_to_use   [n_points] ascending sample sizes in [0, n_reads], 1 <= n_points <= 64;
 *   trials first_trial .. first_trial + n_trials - 1 (32-bit trial numbers), chunk_trials of them at a time on the
 *                  device (0, or more than fit: as many as fit 1 GiB); the result does not depend on it;
 *   out_stats      [n_points][n_trials] x (passed: reads of the sample that carry an index; present: indices with a vote;
 *                  columns_ok: columns the decoder did not give up on, 0 when present is 0; success: present > 0 and the
 *                  decoded data begin with the original file);
 *   out_present, out_payload (each may be NULL): the vote's result, as lva_list_consensus lays it out, per point and trial.
 * Takes a device ordinal like the lva_list_* calls and behaves like them; n_trials = 0 or n_reads = 0 succeeds and
 * touches nothing.
 * ------------------------------------------------------------------------------------------- */
int lva_rs_trials(int32_t device, const int32_t *index, const uint8_t *payload, int32_t n_reads, int32_t bytes_per_oligo,
                  int32_t num_oligos, int32_t redundancy, const uint8_t *original, int64_t original_bytes,
                  const int32_t *reads_to_use, int32_t n_points, uint64_t seed, uint32_t first_trial, int32_t n_trials,
                  int32_t chunk_trials, int32_t *out_stats, uint8_t *out_present, uint8_t *out_payload);

/* ---------------------------------------------------------------------------------------------
 * reads made on the device, in front of lva_transpost_batch_device -- random message ->
 * lva_encode's oligo of the decoder's (mem_conv, rate, msg_len) -> strand -> insertion / deletion / substitution channel
 * -> flip-flop path and dwells -> transition scores in the layout above.  Every draw is a word of Philox4x32-10 under
 * key = seed and counter (item, sub, read number, stream): read number k = first_read + index is the same read in every
 * batch, launch shape and device.  nanopore_dna_storage_amd/simulate.py restates the rules in numpy and is the definition.
 * Shared arguments:
 *   sub_thr, del_thr, ins_thr  floor(p * 2^32) of the channel probabilities, each at most 2^30 (p <= 0.25);
 *   dwell_cdf [dwell_k]        1..64 entries; a base has d extra blocks, d = the first d with word < dwell_cdf[d], else dwell_k;
 *   start_barcode, end_barcode both NULL: the strand is the oligo.  Both given (1..64 characters of ACGT): flank + start
 *                              barcode + oligo + end barcode + flank, flank lengths uniform in [flank_lo, flank_hi],
 *                              flank_hi <= 256, and at most 1024 bases in all;
 *   rc_mode                    0: no strand is reverse-complemented before the channel, 1: all, 2: odd read numbers.
 * first_read + n_reads <= 2^32.  A decoder created with a sync marker is refused with LVA_ERR_UNSUPPORTED (lva_encode
 * takes none).  Refusals in this order, all before the device is touched: own arguments, barcodes, LVA_ERR_BUSY while a
 * decode stream is open, nothing to do (n_reads = 0), device.  Both calls run on the decoder's stream and are complete on
 * return.
 * ------------------------------------------------------------------------------------------- */

/* The lengths-only pass: row_offsets_out / base_offsets_out [n_reads + 1] = block and base offsets of the batch (first 0).
 * LVA_ERR_ARG if the batch exceeds what the other stages take (2^20 blocks per read, 2^31 in all). */
int lva_simulate_plan(lva_decoder *d, uint64_t seed, uint32_t first_read, int32_t n_reads, uint32_t sub_thr, uint32_t del_thr,
                      uint32_t ins_thr, const uint32_t *dwell_cdf, int32_t dwell_k, const char *start_barcode,
                      const char *end_barcode, uint32_t flank_lo, uint32_t flank_hi, int32_t rc_mode, int64_t *row_offsets_out,
                      int64_t *base_offsets_out);
/* The fill pass with the plan's offsets: scores_dev [row_offsets[n_reads]][40] float32 on the decoder's device, 16-byte
 * aligned, = clip(float32(s - 131070) * scale (+ margin on the block's true transition), -clip, clip), s the sum of four
 * 16-bit halves of the noise words; three separately rounded float32 operations.  scale = float32(sigma * sqrt(3) / 65536)
 * gives noise of standard deviation sigma.  clip > 0.  Truth to the host: msgs_out uint8 [n_reads][msg_len]; bases_out
 * uint8 [base_offsets[n_reads]] (0..3, what the channel emitted) and true_idx_out uint8 [row_offsets[n_reads]] (the true
 * transition of every block) or NULL.  Offsets that are not the plan's of the same arguments: LVA_ERR_ARG, with nothing
 * written outside them.  Fewer than 2^32 / 10 blocks.  Afterwards lva_decoder_profile reports total_ms = HIP-event time of
 * the score kernel and read_steps = blocks. */
int lva_simulate_fill_device(lva_decoder *d, uint64_t seed, uint32_t first_read, int32_t n_reads, uint32_t sub_thr,
                             uint32_t del_thr, uint32_t ins_thr, const uint32_t *dwell_cdf, int32_t dwell_k,
                             const char *start_barcode, const char *end_barcode, uint32_t flank_lo, uint32_t flank_hi,
                             int32_t rc_mode, float scale, float margin, float clip, const int64_t *row_offsets,
                             const int64_t *base_offsets, float *scores_dev, uint8_t *msgs_out, uint8_t *bases_out,
                             uint8_t *true_idx_out);

/* The same pair with a pool source: the message of read number k is not drawn bit by bit but is one of n_pool given
 * messages -- the oligos of an encoded file -- chosen by k under the seed (stream 6 of simulate.py: counter (0, 0, k, 6),
 * words w0..w3).  Every other draw of the read is what the pair above makes of the same arguments.
 *   pool [n_pool][msg_len]   host, bytes 0 / 1; 1 <= n_pool <= 2^24 and n_pool * msg_len < 2^31; uploaded per call;
 *   pool_cdf [n_pool]        host, or NULL: entry mulhi(w0, n_pool).  Given: non-decreasing, last entry 0xFFFFFFFF; the
 *                            entry is the first k with w0 < pool_cdf[k], else n_pool - 1, so an entry equal to its
 *                            predecessor is never drawn (uneven coverage: simulate.weights_to_cdf);
 *   rc_mode                  0, 1, 2 as above, 3: the strand is reverse-complemented iff w1 >> 31.
 * A NULL pool, an n_pool outside its range, a pool byte above 1 or a table that decreases or does not end in 0xFFFFFFFF is
 * LVA_ERR_ARG, one of the call's own arguments in the refusal order above (before LVA_ERR_UNSUPPORTED for a sync marker).
 * The fill call also reports what was drawn: source_out int32 [n_reads] (the pool entry) and rc_out uint8 [n_reads] (1: the
 * strand was reverse-complemented), either may be NULL; msgs_out [i] = pool [source_out [i]]. */
int lva_simulate_pool_plan(lva_decoder *d, uint64_t seed, uint32_t first_read, int32_t n_reads, uint32_t sub_thr,
                           uint32_t del_thr, uint32_t ins_thr, const uint32_t *dwell_cdf, int32_t dwell_k,
                           const char *start_barcode, const char *end_barcode, uint32_t flank_lo, uint32_t flank_hi,
                           int32_t rc_mode, const uint8_t *pool, int32_t n_pool, const uint32_t *pool_cdf,
                           int64_t *row_offsets_out, int64_t *base_offsets_out);
int lva_simulate_pool_fill_device(lva_decoder *d, uint64_t seed, uint32_t first_read, int32_t n_reads, uint32_t sub_thr,
                                  uint32_t del_thr, uint32_t ins_thr, const uint32_t *dwell_cdf, int32_t dwell_k,
                                  const char *start_barcode, const char *end_barcode, uint32_t flank_lo, uint32_t flank_hi,
                                  int32_t rc_mode, const uint8_t *pool, int32_t n_pool, const uint32_t *pool_cdf, float scale,
                                  float margin, float clip, const int64_t *row_offsets, const int64_t *base_offsets,
                                  float *scores_dev, uint8_t *msgs_out, uint8_t *bases_out, uint8_t *true_idx_out,
                                  int32_t *source_out, uint8_t *rc_out);

/* ---------------------------------------------------------------------------------------------
 * the error profile of a set of reads -- every read aligned to the oligo it names, its matches,
 * substitutions, deletions and insertions tallied by oligo position.
 * replaces: util/align_compute_stats.sh:45-52 (minimap2 + samtools stats) and util/compile_plot_stats.py (the counts ->
 * <prefix>.error_stats.csv); the mapping step is the index that lva_list_filter accepted, or a simulator's truth.
 * The definition is nanopore_dna_storage_amd/error_profile.py (reference_profile):
 *   a byte is a base if it is A C G T or 0 1 2 3, anything else is N and equals nothing, itself included;
 *   read i is the window bases[first_base[i] .. first_base[i] + n_bases[i]) of one host buffer (windows may overlap),
 *   reverse-complemented first when rc[i] != 0 (N stays N), and is aligned to refs[ref_id[i]] (refs [n_refs][ref_len]);
 *   D is the unit-cost global edit-distance matrix, D[i][0] = i, D[0][j] = j, i over reference positions, j over the window;
 *   the walk starts at (ref_len, n) and takes at (i, j) the first move that applies: diagonal if i, j > 0 and
 *   D[i-1][j-1] + (ref[i-1] != read[j-1]) == D[i][j] (a match or a substitution at position i-1), up if i > 0 and
 *   D[i-1][j] + 1 == D[i][j] (a deletion at position i-1), else left (an insertion in front of position i).
 * Outputs, each may be NULL:
 *   out_read [n_reads][4]     (distance, substitutions, deletions, insertions); a read with ref_id[i] < 0 is skipped: its row
 *                             is four times -1 and it adds nothing below;
 *   out_pos  [ref_len + 1][4] per oligo position (matches, substitutions, deletions, bases inserted in front of it); the first
 *                             three are 0 in row ref_len;
 *   out_conf [4][6]           per reference base A C G T how often it was read as A, C, G, T, N or deleted (a reference N counts
 *                             in no row here, but does in out_pos);
 *   out_ins  [5]              inserted bases by value A C G T N.
 * 1 <= ref_len <= 1024, 0 <= n_bases[i] <= 4096, n_refs >= 1, n_refs * ref_len < 2^31, ref_id[i] < n_refs, first_base[i] >= 0,
 * the sum of n_bases below 2^31; chunk_reads reads at a time on the device (0, or more than fit: as many as fit 1 GiB); the
 * result does not depend on it.  All results are exact integers.  Takes a device ordinal like the lva_list_* calls and
 * behaves like them: arguments first (LVA_ERR_ARG), then n_reads = 0 succeeds and touches nothing, then the device.
 * ------------------------------------------------------------------------------------------- */
int lva_align_profile(int32_t device, const uint8_t *bases, const int64_t *first_base, const int32_t *n_bases, int32_t n_reads,
                      const uint8_t *refs, int32_t n_refs, int32_t ref_len, const int32_t *ref_id,
                      const uint8_t *rc /* NULL: none */, int32_t chunk_reads /* 0: as many as fit 1 GiB */, int32_t *out_read,
                      int64_t *out_pos, int64_t *out_conf, int64_t *out_ins);

/* --- what a GIVEN base sequence scores on a read ---------------------
 * The reference trellis (decode_post_conv_parallel_LVA, :589-858) restricted to one message: a path that carries message M
 * walks M's convolutional states, so what is left is a band of positions x flip-flop states per block -- a forced alignment
 * of the read's posteriors to M's base sequence under the decoder's band, with the reference's two parity buffers that are
 * never cleared.  Every score of a decoded list is one of the two values returned for the listed message, bit for bit.  The
 * definition is nanopore_dna_storage_amd/trellis_score.py (reference_score; message_bases gives the sequence of a message
 * under either rc flag); the kernel is csrc/sc_kernels.hip.
 *   post_dev     a resident posterior buffer (lva_device_upload, lva_transpost_batch_device, the simulator), read i = the
 *                n_blocks[i] blocks from block first_block[i] on, as lva_decode_windows_device takes them;
 *   bases        sequence s = bases[first_base[s] .. + n_bases[s]), codes 0..3 or the characters ACGT, 1 .. 1024 bases each
 *                (the windows of lva_align_profile); the decoder's code does not constrain them: a sequence of n bases has
 *                n + 1 positions, and the band of a pair is lva_band_table's formula for (n_blocks, n + 1, max_deviation);
 *   pairs        int32 [n_pairs][2] = (read, sequence), any order, any number per read;
 *   max_deviation  LVA_MAX_DEVIATION_DEFAULT: the decoder's own; msg_len + mem_conv + 1 or more switches the band off;
 *   out          float [n_pairs][2] = (flip, flop): the scores of the two states of the last base at the last position.
 * Refusals, nothing is launched or allocated: LVA_ERR_ARG for a pair index out of range, a sequence that is empty or longer
 * than 1024, a base that is neither a code 0..3 nor ACGT, a window (paired or not) that is negative, has more than 2^20
 * blocks (the limit of every stage, above) or ends at or beyond block 2^31, and a call whose band tables -- one of n_blocks
 * words per distinct (n_blocks, sequence length) among the pairs -- pass 2^26 words;
 * LVA_ERR_POST_TOO_SHORT for a pair whose window has fewer than n + 2 blocks (the reference's "Too small post matrix");
 * LVA_ERR_BUSY while a decode stream is open.  n_pairs = 0 succeeds and touches nothing.  Posteriors are finite or -inf
 * (NaN and +inf are outside the definition; the device does not look for them and what it returns for such a read is not
 * specified).  The calls run on the decoder's stream, are complete on return and leave
 * the decoder's profile alone.  lva_score_bases takes host posteriors with row_offsets as lva_decode_batch does, uploads
 * them and does the same. */
int lva_score_bases_device(lva_decoder *d, const float *post_dev, const int64_t *first_block, const int64_t *n_blocks,
                           int32_t n_reads, const uint8_t *bases, const int64_t *first_base, const int32_t *n_bases,
                           int32_t n_seqs, const int32_t *pairs, int32_t n_pairs, uint32_t max_deviation, float *out);
int lva_score_bases(lva_decoder *d, const float *post, const int64_t *row_offsets, int32_t n_reads, const uint8_t *bases,
                    const int64_t *first_base, const int32_t *n_bases, int32_t n_seqs, const int32_t *pairs, int32_t n_pairs,
                    uint32_t max_deviation, float *out);

/* The forward score of the same trellis: what ALL alignments of a given base sequence weigh on a read -- the log of the sum,
 * over every path of the one-message trellis, of exp(the path's score).  A softmax of logaddexp(flip, flop) over the entries
 * of a read's list is the posterior of each entry given the read, restricted to the list.  The definition is
 * trellis_score.py (reference_forward; forward_total, list_posterior); the kernel is csrc/fw_kernels.hip.  Arguments,
 * out = float [n_pairs][2] = (flip, flop), refusals and their order are lva_score_bases*'s.  Two differences from the score:
 *   sum for max    every maximum of terms prev + post is m + log(sum exp(term - m)), m the largest term, in the order: a flip
 *                  -- the stay, from flip b2 (if b2 != b), from flop b2 + 4 (at position 1: the stay, then the seven other
 *                  states of position 0 ascending); a flop -- the stay, the step from flip b.  A single finite term is
 *                  returned exactly; all -inf gives -inf, never NaN;
 *   cleared band   a cell outside its block's band is -inf: when block t reads position p or p - 1 of the block before, a
 *                  position outside the band of block t - 1 counts as -inf.  The score's parity buffers that are never
 *                  cleared belong to the reference's Viterbi decoder; a sum over paths that reads a value of two blocks
 *                  earlier again has no meaning.  The result is the weight of the paths that stay inside the band at every
 *                  block; with the band off, the plain forward algorithm.
 * Unlike the score this is a floating-point stage (expf and logf per cell), not bit for bit the definition: the device's
 * error against reference_forward in float64 is held to at most twice the error of the definition's own float32
 * restatement (the same term order, every addition rounded to float32; tests/test_gpu_trellis_forward.py). */
int lva_forward_bases_device(lva_decoder *d, const float *post_dev, const int64_t *first_block, const int64_t *n_blocks,
                             int32_t n_reads, const uint8_t *bases, const int64_t *first_base, const int32_t *n_bases,
                             int32_t n_seqs, const int32_t *pairs, int32_t n_pairs, uint32_t max_deviation, float *out);
int lva_forward_bases(lva_decoder *d, const float *post, const int64_t *row_offsets, int32_t n_reads, const uint8_t *bases,
                      const int64_t *first_base, const int32_t *n_bases, int32_t n_seqs, const int32_t *pairs, int32_t n_pairs,
                      uint32_t max_deviation, float *out);

/* The traceback of the same trellis: WHERE the best path of a given base sequence runs on a read -- a segmentation of the
 * read (the block at which each base begins) and, for a truth that the band cut off, where its path left the band.  The
 * definition is trellis_score.py (reference_trace: the recurrence of reference_score, the predecessor that won recorded per
 * cell -- a later candidate replaces an earlier one only if strictly greater, stay first, then the states below ascending --
 * and the walk back, a position outside a block's band taken from two blocks earlier and counted as a stale hop); the
 * kernels are csrc/st_kernels.hip (st_fill, st_walk).  Arguments as lva_score_bases*, and:
 *   end            the state of the last position the walk starts in: 0 flip, 1 flop, -1 the larger score, flip on a tie;
 *   scratch_limit  bytes of back-pointers on the device at a time (a pair needs n_blocks * min(2 * max_deviation, n + 1),
 *                  rounded up to 16); the pairs go in chunks that fit, one after another; 0: 1 GiB.  The outputs do not
 *                  depend on it;
 *   stride         elements per row of out_enter and out_kind: at least the longest paired sequence;
 *   out_score      float [n_pairs][2] = (flip, flop), lva_score_bases' bits;
 *   out_enter      int32 [n_pairs][stride]: at [p - 1] the block whose transition moved the path into position p, p = 1 .. n;
 *                  the unused tail of a row is -1;
 *   out_kind       uint8 [n_pairs][stride]: 0 if position p was entered and held as flip, 1 as flop; the tail is 255;
 *   out_info       int32 [n_pairs][4] = (end_state 0 / 1, start_state 0 .. 7 at position 0 before the first block, stale hops, 0).
 * A pair whose chosen end score is -inf has no path: its rows are -1 and 255, end_state and start_state -1, stale hops 0.
 * Refusals: lva_score_bases' in its order, then LVA_ERR_ARG for end outside -1 .. 1, a stride below the longest paired
 * sequence, a null output with n_pairs > 0 and a single pair that needs more than scratch_limit -- all before anything is
 * allocated; then LVA_ERR_BUSY while a decode stream is open.  n_pairs = 0 succeeds and touches nothing.  Complete on return;
 * the decoder's profile is left alone. */
int lva_trace_bases_device(lva_decoder *d, const float *post_dev, const int64_t *first_block, const int64_t *n_blocks,
                           int32_t n_reads, const uint8_t *bases, const int64_t *first_base, const int32_t *n_bases,
                           int32_t n_seqs, const int32_t *pairs, int32_t n_pairs, uint32_t max_deviation, int32_t end,
                           uint64_t scratch_limit, int32_t stride, float *out_score, int32_t *out_enter, uint8_t *out_kind,
                           int32_t *out_info);
int lva_trace_bases(lva_decoder *d, const float *post, const int64_t *row_offsets, int32_t n_reads, const uint8_t *bases,
                    const int64_t *first_base, const int32_t *n_bases, int32_t n_seqs, const int32_t *pairs, int32_t n_pairs,
                    uint32_t max_deviation, int32_t end, uint64_t scratch_limit, int32_t stride, float *out_score,
                    int32_t *out_enter, uint8_t *out_kind, int32_t *out_info);


/* ---------------------------------------------------------------------------------------------
 * reads mapped to oligos -- for reads that carry no index of their own (a list that failed the
 * CRC, barcodes that were not found), and for coverage per oligo from real reads.
 * replaces: util/align_compute_stats.sh:21-33 (minimap2 against merged.fa); no agreement with minimap2 is claimed.
 * The definition is nanopore_dna_storage_amd/read_map.py (reference_map); bytes are read as lva_align_profile reads them:
 *   index    the distinct pairs (k-mer, oligo) over every oligo position whose k bases are all bases, 2 bits per base, first
 *            base most significant; a k-mer held by more than max_occ oligos is dropped; ref_len < k: an empty index;
 *   votes    per strand (0: the window, 1: its reverse complement) and oligo, the window positions whose k-mer the oligo holds;
 *   cands    the (strand, oligo) pairs with at least min_votes votes, by (votes descending, strand, oligo): the first `cands`;
 *   dist     D[i][0] = i, D[0][j] = 0, unit costs, oligo rows against window columns: d = min_j D[m][j], e the first such j;
 *   winner   the smallest (d, place among the candidates); second: the smallest d of a candidate with another oligo, or -1;
 *   start    the reversed oligo against window[0:e] reversed, E[i][0] = i, E[0][j] = j: j' the first j with E[m][j] = d.
 * out [n_reads][8] = (ref, best, rc, dist, start, count, votes, second): best the winner's oligo, ref = best if dist <=
 * max_dist, else -1; [start, start + count) the aligned part in the coordinates of the window as given; a read without a
 * candidate: (-1, -1, 0, -1, 0, 0, 0, -1).  The global distance of that part to the oligo is dist, so (start, count, ref,
 * rc) are arguments of lva_align_profile.
 * lva_map_index_create is host-only: 1 <= ref_len <= 1024, 6 <= k <= 12, 1 <= max_occ <= 65535, n_refs >= 1, n_refs *
 * ref_len < 2^31.  lva_map_reads: 1 <= cands <= 8, min_votes >= 1, max_dist >= 0, 0 <= n_bases[i] <= 4096, first_base[i] >=
 * 0, the sum of n_bases below 2^31; chunk_reads reads at a time on the device (0: as many as fit 1 GiB of candidate lists),
 * the result does not depend on it.  Arguments first (LVA_ERR_ARG), then n_reads = 0 succeeds, then the device.
 *
 * A pooled run (merged.fa holds the oligos of every experiment, 108 .. 119 bases): one index over oligos of any lengths,
 * one call for the whole pool.  lva_map_index_create_pooled: oligo o is refs[ref_off[o] .. ref_off[o + 1]); ref_off[0] =
 * 0, ascending, every length in 1 .. 1024, ref_off[n_refs] < 2^31; an oligo shorter than k contributes no k-mer.
 * lva_map_index_create builds the same index for equal lengths.  lva_map_reads refuses an index whose oligos differ in
 * length (LVA_ERR_ARG); lva_map_reads_pooled takes every index: D has rows 0 .. len[o], distances of oligos of different
 * lengths are compared as they are, ref = best if dist <= max_dist[best] (max_dist [n_refs], each >= 0).  With every
 * max_dist equal and min_flank = 0 it returns what lva_map_reads returns.
 *   supplementary pass (min_flank > 0; 0: none, supp is not touched)   of a read with ref >= 0 the longer of the flanks
 *            [0, start) and [start + count, n) of its window, the left one on a tie, if it has at least min_flank bases, is
 *            mapped as a read of its own with the same parameters; supp [n_reads][8] is that mapping's row, its start in
 *            the coordinates of the read's window, and (-1, -1, 0, -1, 0, 0, 0, -1) where there was no pass.  A read whose
 *            supp row has ref >= 0 is chimeric: two oligos in one read.
 * ------------------------------------------------------------------------------------------- */
typedef struct lva_map_index lva_map_index;
/* The same index built on device `device` from the uploaded oligos (csrc/mi_kernels.hip) and resident there until
 * lva_map_index_destroy: the arguments and refusals of lva_map_index_create_pooled (LVA_ERR_ARG, no device looked for), then
 * the device (LVA_ERR_NO_DEVICE).  The call waits for the build: the handle is complete when it returns, nothing of the index
 * is in flight, and a failure leaves *out untouched.  lva_map_reads and lva_map_reads_pooled take such an index with the same
 * `device` and upload the reads alone, with the results of a host-built index; another `device` is LVA_ERR_ARG.  The build
 * orders each list by counting, at a cost of the sum of the squared list lengths: meant for max_occ in the hundreds, not for
 * tens of thousands of oligos that share their k-mers (the host builder sorts and has no such term). */
int lva_map_index_create_device(int32_t device, const uint8_t *refs, const int64_t *ref_off /* [n_refs + 1] */,
                                int32_t n_refs, int32_t k, int32_t max_occ, lva_map_index **out);
/* The tables of an index of either kind, copied to the host -- the same bytes for the same oligos however it was built:
 * offsets[c] .. offsets[c + 1] bound the oligos of k-mer c in lists, ascending; masks as lva_map_reads reads them, ref_len
 * the longest oligo.  pairs: lva_map_index_info. */
int lva_map_index_tables(const lva_map_index *idx, uint32_t *offsets /* [4^k + 1] */, int32_t *lists /* [pairs] */,
                         uint64_t *masks /* [n_refs * 8 * ceil(ref_len / 64)] */);   /* each may be NULL */
int lva_map_index_create_pooled(const uint8_t *refs, const int64_t *ref_off /* [n_refs + 1] */, int32_t n_refs,
                                int32_t k, int32_t max_occ, lva_map_index **out);
int lva_map_reads_pooled(int32_t device, const lva_map_index *idx, const uint8_t *bases, const int64_t *first_base,
                         const int32_t *n_bases, int32_t n_reads, int32_t cands, int32_t min_votes,
                         const int32_t *max_dist /* [n_refs] */, int32_t min_flank, int32_t chunk_reads,
                         int32_t *out /* [n_reads][8] */, int32_t *supp /* [n_reads][8]; may be null iff min_flank == 0 */);
int lva_map_index_create(const uint8_t *refs, int32_t n_refs, int32_t ref_len, int32_t k, int32_t max_occ, lva_map_index **out);
void lva_map_index_destroy(lva_map_index *idx);
/* kept distinct k-mers, kept pairs, k-mers dropped by max_occ; each output may be NULL */
int lva_map_index_info(const lva_map_index *idx, int64_t *kmers, int64_t *pairs, int64_t *dropped_kmers);
int lva_map_reads(int32_t device, const lva_map_index *idx, const uint8_t *bases, const int64_t *first_base, const int32_t *n_bases,
                  int32_t n_reads, int32_t cands, int32_t min_votes, int32_t max_dist,
                  int32_t chunk_reads /* 0: as many as fit */, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif
