/*
 * paxos_batch.h — C ABI of the MI355X batched single-decree ticket-Paxos engine.
 *
 * This is the drop-in boundary for the hot path of rgrover/cloud-haskell-paxos.
 * The reference has NO FFI of its own: its externally visible
 * surface is
 *     server :: Process ()                        /root/reference/src/Server.hs:44
 *     client :: [ProcessId] -> Int -> Process ()  /root/reference/src/Client.hs:85
 * spawned N x / P x by  main  (/root/reference/app/Main.hs:41-46), with the
 * message vocabulary of /root/reference/src/Common.hs:20-68.  A batch driver in
 * app/Main.hs binds the functions below with `foreign import ccall safe`
 * (INTEGRATION.md shows the binding).  Each call runs many independent Paxos
 * instances (N acceptors + P proposers each) under the canonical step schedule
 * of docs/SEMANTICS.md on the GPU and returns the per-instance outcome.
 *
 * Plain C types only.  No C++ exceptions cross this boundary.  All functions
 * return 0 on success or a negative PXB_E_* code.  Protocol failures (panic,
 * stuck, divergence, ...) are DATA in pxb_result.flags, not errors.
 */
#ifndef PAXOS_BATCH_H
#define PAXOS_BATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PXB_ABI_VERSION 5   /* 3: pxb_init / pxb_shutdown, n_bytes bound on wire decode;
                               4: pxb_stream_release, pxb_handoff_counts;
                               5: pxb_reload_hooks, pxb_trace_instance in log mode */

/* ---- error codes ---------------------------------------------------------- */
#define PXB_OK          0
#define PXB_E_INVAL    -1   /* bad config / null pointer / out-of-range field  */
#define PXB_E_HIP      -2   /* HIP runtime error (detail: pxb_last_hip_error)   */
#define PXB_E_OOM      -3   /* device allocation failed                          */
#define PXB_E_NODEV    -4   /* no GPU visible                                    */
#define PXB_E_RCCL     -5   /* collective failure                                */

/* ---- limits of the canonical schedule (docs/SEMANTICS.md §3) ------------ */
#define PXB_MAX_PROPOSERS   3
#define PXB_MIN_ACCEPTORS   2
#define PXB_MAX_ACCEPTORS   9
#define PXB_MAX_DELAY      15
#define PXB_MAX_STEP_CAP 8192
#define PXB_QUEUE_DEPTH     8    /* messages per directed link              */
#define PXB_LOG_TRACK      32    /* log positions checked for divergence    */
#define PXB_TICKET_LIMIT (1 << 14)   /* = the 14-bit ticket fields of the kernel words */
#define PXB_MAX_TICKS    4096    /* log mode: Ticks per proposer            */

/* pxb_config.flags */
#define PXB_CFG_RANDOMIZE 1u     /* config-5 fuzz: per-instance P, loss, delay,
                                    crash drawn from Philox (n_proposers,
                                    loss_ppm, delay_max, crash_ppm are maxima) */
#define PXB_CFG_TRACE_PRODUCTION 2u  /* pxb_trace_instance only (batch runs ignore
                                    it): trace the carry-over variant the batch
                                    kernels run instead of the draining one    */
#define PXB_TRACE_IN_FLIGHT_UNKNOWN 0xFFFFFFFFu  /* trace record: copies of a
                                    broadcast not yet on the links (production
                                    variant), so no end-of-step count          */

/* Everything that defines a batch.  Mirrors the hard-coded constants of the
 * reference (N = 2 acceptors Main.hs:41, P = 2 proposers Main.hs:45, majority
 * rule Client.hs:191-194) plus the new fault schedule. */
typedef struct pxb_config {
  uint64_t seed;             /* Philox key                                     */
  uint64_t first_instance;   /* global id of the first instance (sharding)    */
  uint64_t n_instances;      /* instances in this call                        */
  uint32_t n_proposers;      /* P: 1..3   (clientId = p+1, Client.hs:85)      */
  uint32_t n_acceptors;      /* N: 2..9   (length serverPids, Client.hs:193)  */
  uint32_t loss_ppm;         /* per-message loss probability, ppm             */
  uint32_t delay_max;        /* link delay uniform in [1, delay_max], 1..15   */
  uint32_t crash_ppm;        /* per-acceptor isolation-window probability     */
  uint32_t crash_len_max;    /* window length uniform in [1, crash_len_max]   */
  uint32_t crash_start_max;  /* window start uniform in [0, crash_start_max]  */
  uint32_t skew_max;         /* proposer Tick step uniform in [0, skew_max]   */
  uint32_t step_cap;         /* 1..8192                                        */
  uint32_t flags;            /* PXB_CFG_*                                      */
  /* log mode (ABI 2): the reference's ticker sends a Tick every second,
   * forever (Client.hs:96-100).  n_ticks <= 1 = single decree (one Tick per
   * proposer, at its skew step); n_ticks > 1 = proposer p gets Ticks at steps
   * skew_p + j * tick_period, j = 0..n_ticks-1, and the acceptor logs grow one
   * command per committed slot (Server.hs:73-78). */
  uint32_t n_ticks;          /* 0 / 1 = single decree, else 2..PXB_MAX_TICKS   */
  uint32_t tick_period;      /* steps between Ticks (log mode), 1..8192        */
} pxb_config;

/* Per-instance outcome (16 B).  decided_val is the Command of the first
 * `Execute` broadcast (Client.hs:178) encoded (clientId << 24) | t, i.e.
 * "c<clientId>.<t>" (Client.hs:202-203); 0 = none.  flags bits 0..7 are the
 * PXB_F_* bits, bits 16..31 the number of steps the instance ran. */
typedef struct pxb_result {
  uint32_t decided_val;
  int32_t  decided_ticket;   /* Ticket of that Execute (Common.hs:20)          */
  uint32_t rounds;           /* AskForTicket broadcasts, all proposers         */
  uint32_t flags;
} pxb_result;

#define PXB_F_UNDECIDED       (1u << 0)  /* no Execute ever sent               */
#define PXB_F_STUCK           (1u << 1)  /* quiescent, some proposer not Idle  */
#define PXB_F_PANIC           (1u << 2)  /* Server.hs:76 pattern failure (Q6)  */
#define PXB_F_LOG_DIVERGENCE  (1u << 3)  /* two acceptor logs differ           */
#define PXB_F_STEP_CAP        (1u << 4)
#define PXB_F_QUEUE_OVERFLOW  (1u << 5)
#define PXB_F_TICKET_OVERFLOW (1u << 6)
#define PXB_F_LOG_TRUNC       (1u << 7)  /* a log longer than PXB_LOG_TRACK    */
#define PXB_RESULT_STEPS(f)   ((f) >> 16)

/* Final acceptor record (16 B) — ServerState, Server.hs:24-31.
 * meta = log_len | (dead << 31).  val == 0 means `_proposal = Nothing`. */
typedef struct pxb_acceptor_rec {
  int32_t  t_max;            /* _largestIssuedTicket */
  int32_t  t_store;          /* fst of _proposal     */
  uint32_t val;              /* snd of _proposal     */
  uint32_t meta;
} pxb_acceptor_rec;

/* Run totals (SURVEY.md §8(e) slots 0..7, extended). */
#define PXB_NCOUNTERS 16
enum {
  PXB_C_DECIDED = 0, PXB_C_UNDECIDED, PXB_C_STUCK, PXB_C_PANIC,
  PXB_C_DIVERGENCE, PXB_C_STEP_CAP, PXB_C_ROUNDS, PXB_C_MESSAGES,
  PXB_C_QUEUE_OVERFLOW, PXB_C_TICKET_OVERFLOW, PXB_C_LOG_TRUNC,
  PXB_C_CANON_BYTES,         /* SURVEY.md §8(d) canonical accounting v1       */
  PXB_C_STEPS, PXB_C_INSTANCES,
  PXB_C_EXECUTES,            /* Execute broadcasts (commands committed)       */
  PXB_C_RESERVED15
};
typedef struct pxb_counters { int64_t c[PXB_NCOUNTERS]; } pxb_counters;

/* ---- batch entry points ---------------------------------------------------
 * pxb_run: HOST buffers.  Runs cfg->n_instances instances on the current HIP
 * device, copies the outputs back.  out: n_instances results; log_digest:
 * n_instances * n_acceptors FNV-1a digests (instance-major); acc:
 * n_instances * n_acceptors final acceptor records; totals: run totals.  Every
 * output pointer is nullable.  Blocks until done.
 * Replaces: Main.hs:37-53 (spawn servers/clients, run forever) for a batch.   */
int pxb_run(const pxb_config* cfg, pxb_result* out, uint32_t* log_digest,
            pxb_acceptor_rec* acc, pxb_counters* totals);

/* pxb_run_device: DEVICE buffers, asynchronous on `stream` (a hipStream_t;
 * NULL = default stream).  Same outputs as pxb_run but all pointers are device
 * pointers on the current device.  d_totals (PXB_NCOUNTERS int64) is ADDED to,
 * not overwritten, so many launches can accumulate into one vector.  The
 * batch runs in chunks; each chunk enqueues its kernels and a one-block
 * finalize kernel that folds the chunk's partial totals into d_totals:
 *   fault-free, one proposer, single decree: the fault-free per-lane kernel,
 *     then the general faulty kernel over the instances it handed back
 *     (chunks up to 2^30 - 1);
 *   other fault-free (duelling proposers, log mode): the fault-free per-lane
 *     kernel for those, then the general faulty kernel over its bails;
 *   faulty single decree: the per-lane event kernel, then the general faulty
 *     kernel over its bailed instances; loss-free, skew-free batches with
 *     delays <= 4 (BASELINE config 4) take its simple-schedule shape, and
 *     with two proposers over more than 10 links its tight layout first
 *     (12 waves per CU), the simple-schedule shape over what that hands on;
 *     fuzzed three-proposer batches run the two-proposer event kernel first
 *     and the three-proposer one over the instances that drew P = 3 (chunks
 *     of 2^26; 2^25 split);
 *   faulty log mode (n_ticks > 1, delays <= 8): the per-lane event kernel's
 *     log-mode shape, over <= 10 links the same shape on the 16-step wheel
 *     with a larger pool over what it hands on, then the general log-mode
 *     kernel over the rest (chunks of 2^26; longer delays: the general
 *     log-mode kernel).
 * Each chunk
 * uses one of 64 per-device scratch slots round-robin; a chunk that takes a
 * slot makes its stream wait (on the device, hipStreamWaitEvent) for the
 * event recorded behind the slot's previous chunk, so any number of chunks
 * may be in flight across streams (a 65th waits for the first's slot).  A
 * launch failure after a chunk's first kernel zeroes its slot (behind the
 * queued work) and waits for that work before the error is returned, so
 * nothing of a failed call still touches the caller's buffers.
 * With a digest buffer, the faulty per-lane routings first draw every
 * instance's isolation windows into its digest row (a dense pre-pass kernel);
 * the row holds them until the instance finishes and its digests replace
 * them.  The caller sees digests only, but while a call is in flight nothing
 * else may write its digest buffer, not even the same values.               */
int pxb_run_device(const pxb_config* cfg, pxb_result* d_out, uint32_t* d_log_digest,
                   pxb_acceptor_rec* d_acc, int64_t* d_totals, void* stream);

/* pxb_run_multi: HOST buffers, sharded over devices 0..n_devices-1 (<= 0: all
 * visible) by contiguous global-instance ranges, one host thread per device;
 * totals = one RCCL all-reduce (sum) of the per-device run totals over xGMI.
 * Results are identical to pxb_run for any device count (Philox is keyed by
 * the global instance id).  Concurrent calls from several threads run one
 * after another (they share the cached communicators).
 * Replaces: Main.hs:37-53 for a multi-GPU node.                               */
int pxb_run_multi(const pxb_config* cfg, int n_devices, pxb_result* out, uint32_t* log_digest,
                  pxb_acceptor_rec* acc, pxb_counters* totals);

/* ---- context ------------------------------------------------------------------
 * The library keeps per-device scratch (64 launch slots of partial totals and
 * queue words, 2 MB per device; the wire codec's scan buffer) and the RCCL
 * communicators of pxb_run_multi, created lazily on first use.  The per-lane
 * kernels' bailed-id lists are kept per (device, stream) of pxb_run_device,
 * allocated on that stream's first faulty or per-lane launch: 16 MB each, plus
 * 64 MB for the two-stage routings (config 5's split, config 4's tight), for
 * at most 8 streams per device (a ninth stream takes over the oldest entry:
 * its launches wait on the device for an event recorded behind that entry's
 * last launches, failed chunks included; a stream destroyed by the library
 * hands its entry back).  pxb_init(n) creates the launch slots of devices 0..n-1
 * (n <= 0: all visible) up front; pxb_shutdown() waits for those devices, frees everything
 * and destroys the communicators; the next call starts afresh.  Both are
 * optional.  Do not call pxb_shutdown while other threads have calls in
 * flight.  (A CPU pxb_run_cpu is NOT part of this library: the CPU
 * restatement of the schedule is test infrastructure in oracle/ — the checker
 * and the timed baseline — and the GPU entry points never fall back to it.) */
int pxb_init(int n_devices);
int pxb_shutdown(void);

/* pxb_stream_release (ABI 4): `stream` (a hipStream_t used with pxb_run_device on device
 * `dev`; NULL = the default stream) is about to be destroyed or has no more
 * work for the library: its bailed-id lists go back to the library for the
 * next stream, whose launches first wait (on the device, hipStreamWaitEvent)
 * for the event behind their last launches, even while those still run.
 * Optional (without it a ninth stream takes the oldest entry over the same
 * way); pxb_run_multi calls it for the streams it creates.  Unknown streams
 * are ignored.  First use of a stream allocates its lists: a timed loop should
 * make one small untimed launch on every stream it will use (bench.py does).  */
void pxb_stream_release(int dev, void* stream);

/* ---- per-instance trace (the build counterpart of the reference's `say`
 * state dumps, Server.hs:85 and Client.hs:108) ---------------------------------
 * Runs ONE instance of a single-decree batch on the current device through the
 * per-lane state machine of the faulty kernels (csrc/paxos_ev.h) and records
 * the state at the end of every step it visits: steps with no due message and
 * no Tick change nothing and are skipped (their state is the previous
 * record's).  An instance that ends at the step cap because its next message
 * falls due past it records its last visited step and then, with the same
 * state, the final step step_cap - 1.  Host buffers; out holds max_records records; *n_records is the
 * count written (the last one is the final step); result (nullable) is the
 * instance's pxb_result, as pxb_run gives it.  By default the trace runs the
 * variant of the state machine in which every step sends all of its copies
 * before the next begins, so every record is the schedule's end-of-step state.
 * The batch kernels run a variant that may carry the copies of a step's last
 * broadcast into the next step; with PXB_CFG_TRACE_PRODUCTION in cfg->flags the
 * trace runs that variant instead: records are taken on entering the next step
 * (acceptor and proposer states are the end-of-step ones; in_flight is
 * PXB_TRACE_IN_FLIGHT_UNKNOWN while copies are still to send, and a carried
 * step may be recorded although nothing else falls due in it).
 * Log mode (n_ticks > 1, ABI 5) runs the batch kernels' log-mode shape: the
 * ticker, Execute-driven logs (the acceptor records' log lengths and digests
 * per step) and commands c<id>.<t> in the proposer fields.
 * PXB_E_INVAL for step_cap > 4095, for log mode with delays above 8, or if the
 * instance outgrows the state machine's link capacities (its FIFOs hold 4
 * messages; the batch kernels then hand it to the general kernel) or
 * max_records.                                                               */
typedef struct pxb_trace_prop {
  int32_t  ticket;           /* _ticket                      Client.hs:60    */
  uint32_t cmd;              /* _mCommand, (id << 24) | t or 0 (t = 1 single decree) */
  uint32_t acks;             /* _numAcks                                     */
  uint32_t state;            /* 0 Idle, 1 Round1, 2 Round2                    */
  int32_t  mr_t;             /* Round1: MostRecent (ticket, command)          */
  uint32_t mr_v;
  uint32_t r2_v;             /* Round2: the proposed command                  */
  uint32_t pending;          /* Round2: _originalCommandPending               */
} pxb_trace_prop;
typedef struct pxb_trace_step {
  uint32_t step;             /* the step that just ended                      */
  uint32_t in_flight;        /* messages queued on the links after it         */
  uint32_t n_acceptors, n_proposers;
  pxb_acceptor_rec acc[PXB_MAX_ACCEPTORS];
  uint32_t log_digest[PXB_MAX_ACCEPTORS];
  pxb_trace_prop prop[PXB_MAX_PROPOSERS];
} pxb_trace_step;
int pxb_trace_instance(const pxb_config* cfg, uint64_t instance, pxb_trace_step* out, uint32_t max_records,
                       uint32_t* n_records, pxb_result* result);

/* ---- single-handler hooks (run the kernel's own device functions) -------- */
/* One message in or out.  Requests (ClientRequest, Common.hs:41-45):
 *   kind 0 AskForTicket t | 1 Propose (t, c) | 2 Execute t ; x = t, z = c.
 * Responses (ServerResponse, Common.hs:49-53):
 *   kind 0 Round1OK g (t_store, val) | 1 HaveTicket u | 2 Round2Success ;
 *   x = g or u, y = t_store, z = val.                                        */
typedef struct pxb_msg { uint32_t kind; int32_t x; int32_t y; uint32_t z; } pxb_msg;
#define PXB_MSG_NONE 0xFFFFFFFFu   /* kind of an absent reply */

/* ClientState, Client.hs:58-67 (+ Round1State/Round2State :36-49). */
typedef struct pxb_proposer_rec {
  int32_t  ticket;
  uint32_t cmd;              /* 0 = Nothing          */
  uint32_t acks;
  uint32_t state;            /* 0 Idle, 1 Round1, 2 Round2 */
  int32_t  mr_t;             /* Round1: MostRecent   */
  uint32_t mr_v;
  int32_t  r2_t;             /* Round2: _proposal    */
  uint32_t r2_v;
  uint32_t pending;          /* Round2: _originalCommandPending */
  uint32_t client_id;
} pxb_proposer_rec;

/* handleClientRequest (Server.hs:51-78) applied to count independent
 * (state, message) pairs on the GPU.  reply[i].kind = PXB_MSG_NONE when the
 * handler tells nothing.  A panic (Server.hs:76) sets bit 31 of meta.  Host
 * pointers.                                                                  */
int pxb_acceptor_handle(pxb_acceptor_rec* states, const pxb_msg* req,
                        pxb_msg* reply, uint32_t count);

/* handleServerResponse / handleTick (Client.hs:125-207) applied to count
 * independent (state, message) pairs on the GPU.  msg kind 3 = Tick.  Each
 * handler broadcasts at most two requests (Client.hs:178,185): bcast[2*i],
 * bcast[2*i+1], with n_bcast[i] of them valid.  Host pointers.               */
int pxb_proposer_handle(pxb_proposer_rec* states, uint32_t n_acceptors,
                        const pxb_msg* msg, pxb_msg* bcast, uint32_t* n_bcast,
                        uint32_t count);

/* ---- wire format ----------------------------------------
 * Batch codec for the Data.Binary payloads the reference sends: the generic
 * `instance Binary ClientRequest` / `instance Binary ServerResponse`
 * (Common.hs:24,47,55; binary-0.8.5.1 from the lts-12.18 resolver): Word8
 * constructor tag, Int = Int64 big-endian, Maybe = Word8 0|1 (+ value),
 * Command = Int length + UTF-8 chars of "c<clientId>.<t>".  Messages use
 * pxb_msg: requests kind 0/1/2 with x = ticket, z = command code
 * ((clientId << 24) | t, Propose only); responses kind 0/1/2 with x = ticket,
 * (y, z) = Round1OK's stored proposal (z == 0: Nothing).  A kind above 2
 * encodes to an empty record.  Offsets are exclusive prefix sums
 * (count + 1 entries): message i occupies bytes [off[i], off[i+1]).
 * Replaces: Cloud Haskell's serialisation of `contentOf m` in sendMessages
 * (Common.hs:36-39) for a batch of messages; the envelope (sender ProcessId,
 * type fingerprint, TCP framing) is not part of it.                        */
#define PXB_WIRE_REQUEST   0u     /* ClientRequest  (Common.hs:41-47)        */
#define PXB_WIRE_RESPONSE  1u     /* ServerResponse (Common.hs:49-55)        */
#define PXB_WIRE_MAX_BYTES 39     /* longest record: Round1OK with a Just    */
/* per-message decode status */
#define PXB_WIRE_OK        0u
#define PXB_WIRE_E_LENGTH  1u     /* truncated record or trailing bytes      */
#define PXB_WIRE_E_TAG     2u     /* constructor / Maybe tag out of range    */
#define PXB_WIRE_E_STRING  3u     /* not a "c<id>.<t>" the reference prints  */
#define PXB_WIRE_E_RANGE   4u     /* Int beyond int32, id > 255, t >= 2^24   */

/* DEVICE buffers, asynchronous on `stream`.  pxb_wire_size writes the
 * offsets of `count` encoded messages (d_offsets: count + 1 entries);
 * pxb_wire_encode takes exactly those offsets (it writes the records of each
 * message tile contiguously from the tile's first offset).  Decode
 * accepts any offsets: a record with off[i+1] < off[i] is empty, and one that
 * reaches past n_bytes (the size of d_bytes) is never read; both are
 * PXB_WIRE_E_LENGTH. */
int pxb_wire_size(const pxb_msg* d_msgs, uint64_t count, uint32_t type, uint64_t* d_offsets, void* stream);
int pxb_wire_encode(const pxb_msg* d_msgs, uint64_t count, uint32_t type, const uint64_t* d_offsets,
                    uint8_t* d_bytes, void* stream);
/* size + encode fused: writes the offsets (count + 1 entries) and the records;
 * d_bytes must hold count * PXB_WIRE_MAX_BYTES bytes (or the encoded total).
 * The size / encode_all calls of one device share a scratch buffer: issue
 * them on one stream. */
int pxb_wire_encode_all(const pxb_msg* d_msgs, uint64_t count, uint32_t type, uint64_t* d_offsets,
                        uint8_t* d_bytes, void* stream);
/* d_status (nullable): PXB_WIRE_* per message; failed messages decode to 0s */
int pxb_wire_decode(const uint8_t* d_bytes, uint64_t n_bytes, const uint64_t* d_offsets, uint64_t count,
                    uint32_t type, pxb_msg* d_msgs, uint32_t* d_status, void* stream);
/* HOST-buffer forms (blocking).  encode: `out` holds count * PXB_WIRE_MAX_BYTES
 * bytes, offsets count + 1 entries, *nbytes = total bytes written. */
int pxb_wire_encode_host(const pxb_msg* msgs, uint64_t count, uint32_t type, uint8_t* out, uint64_t* offsets,
                         uint64_t* nbytes);
int pxb_wire_decode_host(const uint8_t* in, uint64_t n_bytes, const uint64_t* offsets, uint64_t count,
                         uint32_t type, pxb_msg* msgs, uint32_t* status);

/* pxb_handoff_counts: instances the per-lane kernels of device `dev` handed on
 * since the device's scratch was created (pxb_init or its first launch) or
 * last reset: out2[0] = by the first per-lane kernel of a chunk (its bails; for
 * the two-stage routings also what the second per-lane kernel re-runs:
 * config 5's P = 3 instances, or config 4's instances that outgrew the tight
 * layout), out2[1] = by a second per-lane kernel (two-stage routings only).
 * What reaches the general kernel is out2[1] for two-stage chunks, out2[0]
 * otherwise.  A list that overflowed counts cap + 1 more.  Waits for the
 * device; reset != 0 zeroes the counts after reading.  Observability only:
 * results never depend on it.                                                */
int pxb_handoff_counts(int dev, uint64_t* out2, int reset);

/* pxb_reload_hooks (ABI 5): re-reads the library's test / A-B hooks from the
 * environment (PXB_NO_EV, PXB_NO_TIGHT, PXB_EV_BAIL_CAP, PXB_BLOCKS_PER_CU, ...:
 * routing and capacity switches the GPU tests use).  They are read once, on
 * pxb_init or the first launch, and then only by this call: the launch path
 * never calls getenv.  Not for production use; unset, nothing changes.       */
void pxb_reload_hooks(void);

/* ---- result queries (additive to ABI 5: PXB_ABI_VERSION is unchanged, callers
 * detect these two entry points by symbol) -----------------------------------
 * Which instances to hand to pxb_trace_instance, and the distributions the run
 * totals only sum, without copying 16 B per instance to the host.             */
#define PXB_Q_ANY   0u   /* (flags & flag_mask) != 0          */
#define PXB_Q_ALL   1u   /* (flags & flag_mask) == flag_mask  */
#define PXB_Q_NONE  2u   /* (flags & flag_mask) == 0          */
#define PXB_HIST_MAX_BINS 8194   /* steps 0..PXB_MAX_STEP_CAP exact, plus one overflow bin */

/* An instance matches when its flags pass the flag test and its steps and
 * rounds both lie in their inclusive ranges (min > max: nothing matches). */
typedef struct pxb_query {      /* 32 B */
  uint32_t flag_mask;           /* PXB_F_* bits only (<= 0xFF)                       */
  uint32_t flag_mode;           /* PXB_Q_*                                           */
  uint32_t steps_min, steps_max;    /* inclusive, on PXB_RESULT_STEPS(flags)         */
  uint32_t rounds_min, rounds_max;  /* inclusive, on pxb_result.rounds               */
  uint32_t n_bins_steps;        /* 0 = no histogram, else 1..PXB_HIST_MAX_BINS       */
  uint32_t n_bins_rounds;
} pxb_query;

/* pxb_query_device: DEVICE buffers, asynchronous on `stream`.  Applies q to
 * d_results[0..count), the results of instances first_instance.. (as
 * pxb_run_device leaves them).  Matches are written in ascending instance
 * order: d_ids[k] = first_instance + index (global ids), d_matched[k]
 * (nullable) the matching record.  *d_n_matches is read as the write cursor
 * and then has the call's full match count added to it, so successive calls on
 * successive chunks append to one list.  Matches whose position is at or past
 * `capacity` are counted but never written, and nothing past `capacity`
 * entries is touched.  The histograms count matching instances only:
 * hist[min(value, n_bins - 1)] += 1, added to what is already there, as
 * d_totals is ({flag_mask = 0, PXB_Q_NONE} with full ranges: everything).
 * All integers: results are bit-reproducible.
 * d_ids may be NULL only when capacity == 0, a histogram pointer only when its
 * n_bins is 0; d_n_matches is required; any count up to 2^40, 0 included.
 * PXB_E_INVAL, before any device call, for a null q, flag_mode > 2,
 * flag_mask > 0xFF, n_bins above PXB_HIST_MAX_BINS or a pointer rule broken.
 * Three passes, and no kernel of the library's that waits for another block:
 * per-tile match counts fused with the histograms, a scan of the tile counts
 * (hipCUB's, as in the wire codec), a scatter that re-reads the tiles that hold
 * matches.  d_results and d_matched are 16-byte aligned (the records move as
 * 16-byte words).  Each call takes its tile counts and offsets
 * (12 B per 1024 results) from the per-device stream-ordered pool of the wire
 * codec, on its own stream: calls on different streams share nothing.         */
int pxb_query_device(const pxb_result* d_results, uint64_t first_instance, uint64_t count,
                     const pxb_query* q,
                     uint64_t* d_ids, pxb_result* d_matched, uint64_t capacity,
                     uint64_t* d_n_matches,
                     int64_t* d_hist_steps, int64_t* d_hist_rounds, void* stream);

/* pxb_sweep: HOST buffers, blocking, on the current device.  Runs
 * cfg->n_instances instances in chunks of at most 2^24 (one pxb_run_device
 * each, no digests or acceptor records, into one reused result buffer) and
 * queries each chunk on the device with a running cursor, so only the match
 * list, the bins and the totals cross to the host.  *n_matches (the full match
 * count) and the histograms (n_bins entries each) are OVERWRITTEN; ids and
 * matched (nullable) hold `capacity` entries: the smallest matching ids;
 * totals (nullable) are pxb_run's.  The answer is exactly the query applied on
 * the host to pxb_run's results.
 * Device memory, whatever n_instances is: one chunk of results (16 B x
 * min(n_instances, 2^24) = 256 MiB at most, + 12 B per 1024 of them while a
 * query runs) + min(capacity, n_instances) x 24 B (16 without `matched`) +
 * 8 B x the bins + the run's own per-device scratch.
 * Validation as pxb_query_device's and pxb_run's; PXB_E_NODEV without a GPU.
 * (PXB_SWEEP_CHUNK, a test hook read like the others, clamped to
 * [1, 2^30 - 1], sets the chunk size.)                                        */
int pxb_sweep(const pxb_config* cfg, const pxb_query* q,
              uint64_t* ids, pxb_result* matched, uint64_t capacity, uint64_t* n_matches,
              int64_t* hist_steps, int64_t* hist_rounds, pxb_counters* totals);

/* ---- batched trace (additive to ABI 5, found by symbol like the queries) ------
 * The instances a sweep lists, traced in one launch: ids in, per-step records
 * out, on the device.  Let R(id) be the records pxb_trace_instance(cfg, id, ...)
 * returns with enough max_records (the same variant: default, or
 * PXB_CFG_TRACE_PRODUCTION in cfg->flags; log mode when n_ticks > 1), and
 * kept(id) those of R(id) whose step lies in [step_min, step_max], cut to the
 * last `tail` of them when tail != 0.  Then
 *   d_offsets[i]  = sum of |kept(d_ids[j])| over j < i   (count + 1 entries;
 *                   d_offsets[count] is the total),
 *   d_records[d_offsets[i] ...] = kept(d_ids[i]) in step order, byte for byte
 *                   the pxb_trace_step records pxb_trace_instance writes,
 *   d_status[i]   = PXB_TRACE_OK, or PXB_TRACE_BAILED for an instance that
 *                   outgrew the per-lane state machine's link capacities (where
 *                   pxb_trace_instance returns PXB_E_INVAL): kept is empty and
 *                   d_results[i] is zeroed,
 *   d_results[i]  = the instance's pxb_result, as pxb_run gives it.
 * Output follows the order of d_ids: ids may be unsorted, repeated and on both
 * sides of 2^32; cfg->first_instance and cfg->n_instances are ignored.  A record
 * whose position is at or past `capacity` is counted in the offsets but not
 * written, and nothing at or past `capacity` entries is touched.  d_records may
 * be NULL only when capacity == 0: the sizing call (offsets, status and results
 * only; the record-writing pass does not run).  d_status and d_results are
 * nullable, d_offsets is required.  Asynchronous on `stream`, no device
 * synchronisation.  PXB_E_INVAL, before any device call, for a null cfg or
 * d_offsets, a null d_ids with count > 0, count > 2^30, sel->reserved != 0,
 * d_records == NULL with capacity > 0, and every config pxb_trace_instance
 * rejects.  count == 0 is valid and writes d_offsets[0] = 0.
 * Two passes of one kernel (one 64-lane wave per block, lane l of block b runs
 * d_ids[64 b + l]) with hipCUB's exclusive sum between them: the first counts,
 * the second re-runs the (deterministic) instances and writes; no block waits
 * for another.  Scratch (4 B per id + the scan's) comes from the per-device
 * stream-ordered pool of the wire codec and the query, on the caller's stream. */
#define PXB_TRACE_OK      0u
#define PXB_TRACE_BAILED  1u   /* outgrew the per-lane state machine's link capacities
                                  (where pxb_trace_instance returns PXB_E_INVAL): no records */
typedef struct pxb_trace_sel {   /* 16 B; NULL = every record */
  uint32_t step_min, step_max;   /* keep records with step_min <= step <= step_max (min > max: none) */
  uint32_t tail;                 /* != 0: of those, only the last `tail` per instance */
  uint32_t reserved;             /* must be 0 */
} pxb_trace_sel;

int pxb_trace_batch_device(const pxb_config* cfg, const uint64_t* d_ids, uint64_t count,
                           const pxb_trace_sel* sel,
                           pxb_trace_step* d_records, uint64_t capacity,
                           uint64_t* d_offsets,      /* count + 1 entries, required */
                           uint32_t* d_status,       /* count, nullable */
                           pxb_result* d_results,    /* count, nullable */
                           void* stream);
/* pxb_trace_batch: HOST buffers, blocking, on the current device; PXB_E_NODEV
 * without a GPU (checked after the validation above).  Runs the count pass,
 * reads the total, and allocates min(total, capacity) records on the device,
 * not `capacity`; *n_records (nullable) is the full total.                    */
int pxb_trace_batch(const pxb_config* cfg, const uint64_t* ids, uint64_t count, const pxb_trace_sel* sel,
                    pxb_trace_step* records, uint64_t capacity, uint64_t* offsets,
                    uint32_t* status, pxb_result* results, uint64_t* n_records);

/* ---- scripted schedules (additive to ABI 5, found by symbol like the queries) --
 * The fault schedule as data (docs/SEMANTICS.md §10): a script ROW is one
 * instance, a Philox base id plus overrides of its schedule draws.  Every field
 * has a "keep" value that takes what Philox gives (cfg->seed, base), so a row of
 * all "keep" is the instance `base`, and a fully explicit row (what
 * pxb_schedule_extract writes) runs the same under any seed and base as long as
 * no link consumes more than `depth` entries.
 * For a call with P = cfg->n_proposers, N = cfg->n_acceptors and depth
 * (0..PXB_SCRIPT_MAX_DEPTH), rows sit pxb_script_stride(P, N, depth) bytes apart
 * (a multiple of 8; the rows are 8-byte aligned), little-endian:
 *   offset  field
 *   0       uint64 base            Philox counter id
 *   8       uint8  n_proposers     0 = keep, else 1..P: overrides what
 *                                  PXB_CFG_RANDOMIZE drew (or cfg->n_proposers)
 *   9       uint8  reserved        must be 0
 *   10      uint16 skew[3]         Tick step of proposer p; 0xFFFF = keep
 *   16      N x {uint16 c0, c1}    isolation window [c0, c1) of acceptor a; both
 *                                  0xFFFF = keep; c0 >= c1 = none; values clamp
 *                                  to 4096 (steps are < 4095)
 *   16+4N   uint8 link[2][P][N][depth]   [dirn][p][a][k]: the §4 message draw of
 *                                  link (dirn, p, a) (dirn 0: p -> a, 1: a -> p),
 *                                  seq k.  0xFF = keep, 0 = lost, 1..0xFE =
 *                                  delivered with delay min(byte, cfg->delay_max)
 *   ...     zero padding to the stride
 * Seq k >= depth is always "keep".  A bad row (n_proposers > P, reserved != 0)
 * gives status PXB_SCRIPT_BAD, a zeroed result and no records; its neighbours
 * are unaffected.  An instance that outgrows the per-lane state machine's link
 * capacities gives PXB_TRACE_BAILED, as in pxb_trace_batch: scripted runs never
 * reach the general kernel.  cfg->first_instance and cfg->n_instances are
 * ignored.  All three device calls are asynchronous on `stream` with no device
 * synchronisation; the run and the trace launch one 64-lane wave per block
 * (lane l of block b runs row 64 b + l), no block waits for another, and the
 * trace takes its scratch (4 B per row + the scan's) from the per-device
 * stream-ordered pool of the wire codec on that stream (the others need none).
 * PXB_E_INVAL, before any device call, for a null cfg, null rows (ids, offsets)
 * with count > 0, depth > PXB_SCRIPT_MAX_DEPTH, count > 2^30 and every config
 * pxb_trace_instance rejects; the host forms return PXB_E_NODEV afterwards
 * without a GPU.                                                              */
#define PXB_SCRIPT_MAX_DEPTH 4096u
#define PXB_SCRIPT_BAD       2u   /* status: malformed row (not run)            */
#define PXB_SCRIPT_KEEP8     0xFFu
#define PXB_SCRIPT_KEEP16    0xFFFFu
/* the first 16 bytes of a row; the windows follow, then the link table */
typedef struct pxb_script_head {
  uint64_t base;
  uint8_t  n_proposers;
  uint8_t  reserved;
  uint16_t skew[PXB_MAX_PROPOSERS];
} pxb_script_head;
typedef struct pxb_script_window { uint16_t c0, c1; } pxb_script_window;
#define PXB_SCRIPT_WINDOWS_OFF    16u                        /* = sizeof(pxb_script_head) */
#define PXB_SCRIPT_LINKS_OFF(n_acceptors) (16u + 4u * (n_acceptors))
uint64_t pxb_script_stride(uint32_t n_proposers, uint32_t n_acceptors, uint32_t depth);

/* pxb_schedule_extract: the schedule Philox gives (cfg->seed, ids[i]) as fully
 * explicit rows, no "keep" anywhere: the drawn P (under PXB_CFG_RANDOMIZE), the
 * skews, the windows (as window_of clamps them; none = 0, 0) and every link
 * byte of the proposers the instance has.  Links of absent proposers are 0xFF
 * (never read), their skews 0.  A dense kernel, one thread per row byte; pure
 * Philox, no state machine runs.                                             */
int pxb_schedule_extract_device(const pxb_config* cfg, const uint64_t* d_ids, uint64_t count, uint32_t depth,
                                uint8_t* d_rows, void* stream);
int pxb_schedule_extract(const pxb_config* cfg, const uint64_t* ids, uint64_t count, uint32_t depth, uint8_t* rows);

/* pxb_run_scripted: the rows through the per-lane state machine; outputs as
 * pxb_run's, row by row (d_out count results, d_log_digest and d_acc count * N;
 * all nullable), d_status (nullable) PXB_TRACE_OK / PXB_TRACE_BAILED /
 * PXB_SCRIPT_BAD (not OK: zeroed outputs), and d_sent (nullable, count x 2 P N
 * uint16, link order as in the row): the messages sent on each link, i.e. the
 * seqs consumed, which tell which entries mattered and whether depth covered
 * the run.  No run totals: pxb_query_device works on d_out.                   */
int pxb_run_scripted_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                            pxb_result* d_out, uint32_t* d_log_digest, pxb_acceptor_rec* d_acc,
                            uint32_t* d_status, uint16_t* d_sent, void* stream);
int pxb_run_scripted(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                     pxb_result* out, uint32_t* log_digest, pxb_acceptor_rec* acc, uint32_t* status,
                     uint16_t* sent);

/* pxb_trace_scripted: pxb_trace_batch with rows in place of ids: the same
 * selection, offsets, capacity and sizing rules, and the same record bytes.
 * The default (end-of-step) variant only: PXB_CFG_TRACE_PRODUCTION is
 * PXB_E_INVAL.  Log mode as in pxb_trace_batch.                               */
int pxb_trace_scripted_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                              const pxb_trace_sel* sel, pxb_trace_step* d_records, uint64_t capacity,
                              uint64_t* d_offsets, uint32_t* d_status, pxb_result* d_results, void* stream);
int pxb_trace_scripted(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                       const pxb_trace_sel* sel, pxb_trace_step* records, uint64_t capacity, uint64_t* offsets,
                       uint32_t* status, pxb_result* results, uint64_t* n_records);

/* ---- handler events of scripted rows (additive to ABI 5, found by symbol) -------
 * pxb_trace_events: one record per handler invocation of a script row, at the
 * granularity of the reference's `say` lines (Server.hs:85, Client.hs:108: the
 * state after every handled message; the commented-out Server.hs:86 and
 * Client.hs:109: the messages the handler sends), for many rows at once
 * (docs/SEMANTICS.md §13).  pxb_trace_scripted tells the state at the end of
 * each step; this tells which message was handled, by whom, and what it
 * produced.  An all-keep row at depth 0 with base = id is the plain instance id.
 * Messages are pxb_msg as pxb_acceptor_handle / pxb_proposer_handle take them:
 * requests kind 0/1/2 with x = ticket, z = command (Propose only); responses
 * kind 0/1/2 with x, (y, z) = Round1OK's stored proposal; a Tick is kind 3.
 * Commands are (clientId << 24) | t, in single-decree and in log mode.
 * An acceptor's out[0] is its reply.  A proposer's out[] are its broadcasts in
 * order, the handler's own and then the restart's AskForTicket (Client.hs:185),
 * each listed once, not once per copy.  after.acc / after.prop are what
 * pxb_trace_step.acc[a], .log_digest[a] / .prop[p] would hold at that moment.
 * A request that reaches a dead or an isolated acceptor is discarded: n_out = 0,
 * the state unchanged; dead is told before isolated.
 * A row's events come in the order of the reference model's pops: by step; in a
 * step the acceptor phase (a ascending, then p ascending, then the link's FIFO
 * order), then the proposer phase (p ascending: its Tick, then a ascending, then
 * FIFO order).  sel->step_min..step_max select by event.step; sel->tail and
 * sel->reserved must be 0.  Offsets (count + 1 entries, events), capacity,
 * the sizing call (d_events NULL with capacity 0), d_status and d_results
 * (both nullable), alignment (events 16 bytes), scratch and the call rules are
 * pxb_trace_scripted's: events at or past `capacity` are counted and never
 * written, and nothing at or past `capacity` entries is touched; a row that is
 * not PXB_TRACE_OK has no events and a zeroed result.  The default variant only
 * (PXB_CFG_TRACE_PRODUCTION: PXB_E_INVAL).  The write pass stages the first
 * min(total, capacity + 256) events and a dense kernel, one thread per staged
 * event, puts each in its canonical place (a row's step holds at most 246
 * events).  The device form cannot know the total without a synchronise, so
 * with capacity > 0 it ALLOCATES a staging buffer of capacity + 256 events
 * (96 B each) from the stream-ordered pool, whatever the total: pass the
 * sizing call's total as capacity, not a generous upper bound (a staging
 * buffer that cannot be allocated is PXB_E_OOM).  The host form does so: it
 * allocates min(total, capacity) events on the device.                        */
#define PXB_EVT_ACCEPTOR 0u
#define PXB_EVT_PROPOSER 1u
#define PXB_EVT_HANDLED          0u
#define PXB_EVT_DISCARDED_DEAD   1u   /* acceptor dead (after a panic): no handler ran  */
#define PXB_EVT_DISCARDED_ISOL   2u   /* acceptor alive but inside its isolation window */
#define PXB_EVT_PEER_TICK     0xFFu
typedef struct pxb_trace_event {      /* 96 B, 16-byte aligned, no implicit padding */
  uint32_t step;
  uint8_t  actor;            /* PXB_EVT_ACCEPTOR / PXB_EVT_PROPOSER                          */
  uint8_t  index;            /* a, or p                                                      */
  uint8_t  peer;             /* the sender: p for an acceptor event, a for a proposer event, */
                             /* PXB_EVT_PEER_TICK for a Tick                                 */
  uint8_t  fate;             /* PXB_EVT_HANDLED / _DISCARDED_*                               */
  uint32_t n_out;            /* messages the handler produced: 0..1 (acceptor), 0..2 (proposer) */
  uint32_t reserved;         /* 0                                                            */
  pxb_msg  in;               /* the message handled                                          */
  pxb_msg  out[2];           /* produced messages; unused entries all 0                      */
  union {                    /* the actor's state AFTER the handler; 32 B, unused bytes 0    */
    struct { pxb_acceptor_rec rec; uint32_t log_digest; } acc;
    pxb_trace_prop prop;
  } after;
} pxb_trace_event;
int pxb_trace_events_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                            const pxb_trace_sel* sel, pxb_trace_event* d_events, uint64_t capacity,
                            uint64_t* d_offsets, uint32_t* d_status, pxb_result* d_results, void* stream);
int pxb_trace_events(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                     const pxb_trace_sel* sel, pxb_trace_event* events, uint64_t capacity, uint64_t* offsets,
                     uint32_t* status, pxb_result* results, uint64_t* n_events);

/* ---- handler-path coverage (additive to ABI 5, found by symbol) -----------------
 * pxb_cover: which handler paths and reference quirks a script row exercised
 * (docs/SEMANTICS.md §14).  The coverage mask of a row is the OR of the classes
 * below over the row's events (pxb_trace_events); a row that is not
 * PXB_TRACE_OK has mask 0, a zeroed result, and counts under rows_bailed /
 * rows_bad only.  Each class depends on the event and on the earlier events of
 * the same actor; the table with the exact conditions is §14's, and
 * pxb.cover_of_events is its executable form.  Nothing is stored per event: the
 * kernels run pxb_trace_events' lane and fold its events in registers.
 *
 * The summary: count[b] = the OK rows with class b; witness[b] = among those
 * the row with the fewest steps (result.flags >> 16), ties to the lowest i: its
 * row index (rows forms) or its instance id first + i (range form), with its
 * steps in witness_steps[b]; both all ones (~0) when count[b] == 0, and for
 * b >= PXB_COVER_CLASSES.  union_mask = the classes with count[b] != 0.
 * Integer adds and minima only: the summary does not depend on the launch.
 *
 * pxb_cover_device: d_rows as pxb_trace_events_device takes them (count <=
 * 2^30, pxb_script_stride(P, N, depth) apart, 8-byte aligned); d_masks,
 * d_status, d_results (16-byte aligned) and d_summary (8-byte aligned) are all
 * nullable.  Asynchronous on `stream`, no device synchronisation, no
 * allocation.  n_matches is 0.  count == 0 gives the empty summary.
 * pxb_cover: the same over host buffers.
 *
 * pxb_cover_range: the plain instances first + i, i < count (ids wrap modulo
 * 2^64), run as all-keep rows at depth 0 in chunks of `chunk` ids (0: 2^20; at
 * most 2^30); device memory is one chunk of rows, masks and status from the
 * stream-ordered pool plus the match list, whatever `count` is.  With a query q,
 * a row MATCHES when it is PXB_TRACE_OK, (m & all_mask) == all_mask, any_mask
 * == 0 or (m & any_mask) != 0, and (m & none_mask) == 0; n_matches counts every
 * match and match_ids / match_masks (nullable; match_ids required when
 * max_matches > 0) get the first max_matches in ascending i.  q == NULL: no
 * list, n_matches = 0.  No output depends on `chunk`.
 *
 * PXB_E_INVAL, decided before any device call: a null cfg, null rows with
 * count > 0, count > 2^30 (rows forms), chunk > 2^30, depth > 4096, a misaligned
 * device pointer, q->reserved != 0, PXB_CFG_TRACE_PRODUCTION, and every config
 * pxb_trace_instance rejects.  The host forms then return PXB_E_NODEV without
 * a GPU.                                                                       */
#define PXB_COVER_CLASSES 29
#define PXB_COVER_ASK_GRANT_EMPTY      (1u << 0)   /* acceptor: Ask -> Round1OK(Nothing)            */
#define PXB_COVER_ASK_GRANT_STORED     (1u << 1)   /* Ask -> Round1OK with a stored proposal         */
#define PXB_COVER_ASK_NACK             (1u << 2)   /* Ask -> HaveTicket                              */
#define PXB_COVER_PROPOSE_ACCEPT       (1u << 3)   /* Propose -> Round2Success                       */
#define PXB_COVER_PROPOSE_NACK         (1u << 4)   /* Propose -> HaveTicket                          */
#define PXB_COVER_EXEC_APPLY           (1u << 5)   /* Execute, the log grew                          */
#define PXB_COVER_EXEC_IGNORED         (1u << 6)   /* Execute, alive after, log unchanged            */
#define PXB_COVER_EXEC_PANIC           (1u << 7)   /* Execute, dead after (Q6)                       */
#define PXB_COVER_DISCARD_DEAD         (1u << 8)   /* discarded: dead                                */
#define PXB_COVER_DISCARD_ISOLATED     (1u << 9)   /* discarded: isolated                            */
#define PXB_COVER_Q1_FOREIGN_ACCEPT    (1u << 10)  /* accepted from a proposer it did not grant last */
#define PXB_COVER_Q7_STALE_EXEC        (1u << 11)  /* applied a proposal that was not fresh          */
#define PXB_COVER_TICK_START           (1u << 12)  /* proposer: Tick with an output                  */
#define PXB_COVER_TICK_BUSY            (1u << 13)  /* Tick without one                               */
#define PXB_COVER_HAVE_IDLE            (1u << 14)  /* HaveTicket, before Idle                        */
#define PXB_COVER_HAVE_BELOW           (1u << 15)  /* HaveTicket, before not Idle, no output         */
#define PXB_COVER_HAVE_RESTART_R1      (1u << 16)  /* HaveTicket with output, before Round1          */
#define PXB_COVER_HAVE_ABORT_R2        (1u << 17)  /* HaveTicket with output, before Round2 (Q10)    */
#define PXB_COVER_R1OK_STALE           (1u << 18)  /* Round1OK not counted                           */
#define PXB_COVER_R1OK_ACK             (1u << 19)  /* counted, no output                             */
#define PXB_COVER_R1OK_PROPOSE_OWN     (1u << 20)  /* counted, Propose, after.pending == 0           */
#define PXB_COVER_R1OK_PROPOSE_ADOPTED (1u << 21)  /* counted, Propose, after.pending != 0           */
#define PXB_COVER_Q5_ADOPTED_OWN       (1u << 22)  /* bit 21 with after.r2_v == after.cmd            */
#define PXB_COVER_Q4_TIE               (1u << 23)  /* counted Round1OK whose ticket ties the MostRecent */
#define PXB_COVER_R2S_DROPPED          (1u << 24)  /* Round2Success, before not Round2               */
#define PXB_COVER_R2S_ACK              (1u << 25)  /* counted, no output                             */
#define PXB_COVER_R2S_DONE             (1u << 26)  /* counted, Execute                               */
#define PXB_COVER_R2S_RESTART          (1u << 27)  /* counted, Execute then AskForTicket             */
#define PXB_COVER_R2S_REPEAT           (1u << 28)  /* counted twice from one acceptor in one Round 2 (Q2/Q3) */
typedef struct pxb_cover_summary {    /* 680 B, no implicit padding */
  uint64_t rows_ok, rows_bailed, rows_bad, n_matches;
  uint64_t count[32];          /* OK rows with class b                                   */
  uint64_t witness[32];        /* row index (rows form) or global id (range form) of the  */
  uint32_t witness_steps[32];  /* OK row with class b that has the fewest steps, lowest i */
  uint32_t union_mask, reserved;       /* among those; ~0 / 0xFFFFFFFF when count[b] == 0 */
} pxb_cover_summary;
typedef struct pxb_cover_query { uint32_t all_mask, any_mask, none_mask, reserved; } pxb_cover_query;
int pxb_cover_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                     uint32_t* d_masks, uint32_t* d_status, pxb_result* d_results,
                     pxb_cover_summary* d_summary, void* stream);
int pxb_cover(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
              uint32_t* masks, uint32_t* status, pxb_result* results, pxb_cover_summary* summary);
int pxb_cover_range(const pxb_config* cfg, uint64_t first, uint64_t count, uint64_t chunk /* 0: default 2^20 */,
                    const pxb_cover_query* q /* nullable: no list */, uint64_t* match_ids, uint32_t* match_masks,
                    uint64_t max_matches, pxb_cover_summary* summary);

/* ---- batched shrinker (additive to ABI 5, found by symbol like the queries) ----
 * Many failing schedules reduced to 1-minimal fault sets at once, everything on
 * the device (docs/SEMANTICS.md §11).  Row i of d_rows (fully explicit rows, as
 * pxb_schedule_extract writes them, pxb_script_stride apart) is shrunk in place.
 * The PREDICATE of a run is: status PXB_TRACE_OK, result.flags & 0xFF &
 * flag_mask != 0, and no link consumed more than `depth` entries.  A FAULT of a
 * row, given its run's send counts, is a non-zero skew of a proposer the row
 * has, a non-empty window, or a consumed link entry (k < min(sent, depth)) that
 * is lost or delayed by more than one step; neutralising sets it to 0, none or
 * 1.  Per row, launch 1 runs the row itself; then rounds of two launches while
 * faults remain and launches + 2 <= max_launches: every single neutralisation
 * (if none holds the row is 1-minimal: that launch is the proof), then every
 * prefix of the removable faults, of which the longest that holds is taken
 * with its send counts.  After every accepted row, link entries at k >= sent
 * become 1 and the others that are neither 0 nor 0xFF are clamped to
 * cfg->delay_max.  Rows run in lockstep and do not influence each other: a
 * row's outputs do not depend on the batch, its position in it or repeats.
 * Outputs (all nullable), per row:
 *   d_status     PXB_SHRINK_*
 *   d_n_faults   faults left in the returned row
 *   d_launches   launches that row took part in (the initial one included)
 *   d_sent       2 P N uint16, the returned row's send counts (link order)
 *   d_results    the returned row's pxb_result (NOT_INPUT / TOO_MANY: the given row's)
 *   d_signature  FNV-1a-64 (basis 0xCBF29CE484222325, prime 0x100000001B3) over the
 *                row's n_proposers byte, then 8 bytes per fault in ascending
 *                row offset, little-endian: skew (0, 0, p, 0, skew u16, 0 u16),
 *                window (1, 0, 0, a, c0 u16, c1 u16; as clamped to 4096),
 *                link (2, dirn, p, a, k u16, byte u16).  Equal signatures: the
 *                same minimal schedule.
 * NOT_INPUT and TOO_MANY leave the row as given, with launches 1, n_faults 0,
 * sent and signature 0.
 * No candidate row is ever stored: a candidate is its parent's row read through
 * a uint16 rank table (one entry per skew, window and link byte), so scratch is
 * count x (2 x stride + 2 x entries) plus, per launch, 1 B per candidate (and
 * 4 P N + 16 B in the initial and prefix launches), all from the per-device
 * stream-ordered pool on `stream`.  The rows are shrunk in a scratch copy and
 * written back at the end: a call that fails (PXB_E_OOM for a failed
 * allocation) has written nothing.  The host loop reads one 8-byte candidate
 * total per launch to size the next grid, so the device form SYNCHRONISES ITS
 * STREAM once per launch, at most 1 + 2 ceil((max_launches - 1) / 2) times.
 * PXB_E_INVAL, before any device call, for a null cfg, null rows with count >
 * 0, depth > PXB_SCRIPT_MAX_DEPTH, count > 2^30, flag_mask & 0xFF == 0,
 * max_launches == 0, buffers misaligned for their element (rows 8, results
 * 16), and every config pxb_trace_instance rejects.  count == 0 is valid.    */
#define PXB_SHRINK_MINIMAL    0u   /* 1-minimal, or no faults at all                      */
#define PXB_SHRINK_BUDGET     1u   /* stopped by max_launches: the last accepted row      */
#define PXB_SHRINK_NOT_INPUT  2u   /* the given row does not hold the predicate           */
#define PXB_SHRINK_TOO_MANY   3u   /* more than 65,534 faults: treated as NOT_INPUT       */
#define PXB_SHRINK_UNSTABLE   4u   /* no prefix held (deterministic runs never give it)   */
int pxb_shrink_batch_device(const pxb_config* cfg, uint8_t* d_rows, uint64_t count, uint32_t depth,
                            uint32_t flag_mask, uint32_t max_launches,
                            uint32_t* d_status, uint32_t* d_n_faults, uint32_t* d_launches,
                            uint16_t* d_sent, pxb_result* d_results, uint64_t* d_signature, void* stream);
/* pxb_shrink_batch: HOST buffers, blocking, on the current device; PXB_E_NODEV
 * without a GPU (checked after the validation above).  ids non-null: rows is
 * output only, the schedules of ids[i] are extracted on the device first.    */
int pxb_shrink_batch(const pxb_config* cfg, const uint64_t* ids, uint8_t* rows, uint64_t count, uint32_t depth,
                     uint32_t flag_mask, uint32_t max_launches,
                     uint32_t* status, uint32_t* n_faults, uint32_t* launches,
                     uint16_t* sent, pxb_result* results, uint64_t* signature);

/* ---- exploration (additive to ABI 5, found by symbol like the queries) ---------
 * Every schedule within `radius` changed link entries of a row, run on the
 * device (docs/SEMANTICS.md §12).  With P = cfg->n_proposers, N =
 * cfg->n_acceptors and A = cfg->delay_max, the SITES of a row are the first
 * site_depth entries of every link: S = 2 P N site_depth, site s = link
 * s / site_depth (the row's link order, (dirn P + p) N + a), seq
 * s % site_depth.  Skews and windows are not sites; a parent may carry any.
 * Digit j (0..A-1) of a site whose parent byte is b reads as
 * (min(b, A) + 1 + j) mod (A + 1): every value in 0..A (0: lost) but the
 * parent's own.  With n_r = C(S, r) A^r and base_r the sum of n_q over q < r,
 * a parent has T = base_(radius + 1) candidates; candidate c in [base_r,
 * base_(r+1)), x = c - base_r, changes the r sites s_1 < .. < s_r with
 * x / A^r = sum of C(s_i, i) (the combinatorial number system), site s_i taking
 * digit (x % A^r / A^(i-1)) % A.  Candidate 0 is the parent itself.  A candidate
 * that changes a site whose parent byte is 0xFF (keep; the links of absent
 * proposers in extracted rows) is SKIPPED: it does not run, did not run OK and
 * never holds.  A candidate HOLDS by the shrinker's predicate: status
 * PXB_TRACE_OK, result.flags & 0xFF & flag_mask != 0 and no link consumed more
 * than `depth` entries.  A held candidate is MINIMAL when no candidate made of
 * a proper subset of its changes (same digits; candidate 0 included) holds.   */
#define PXB_EXPLORE_MAX_RADIUS 3u
#define PXB_EXPLORE_MINIMAL    1u   /* list only minimal candidates */
typedef struct pxb_explore_space {  /* 16 B */
  uint32_t site_depth;              /* 1..depth                                    */
  uint32_t radius;                  /* 0..PXB_EXPLORE_MAX_RADIUS                   */
  uint32_t flag_mask;               /* PXB_F_* bits of the predicate (& 0xFF != 0) */
  uint32_t flags;                   /* PXB_EXPLORE_MINIMAL or 0                    */
} pxb_explore_space;

/* T, or 0 for a space that is invalid or larger than 2^30 candidates. */
uint64_t pxb_explore_total(uint32_t n_proposers, uint32_t n_acceptors, uint32_t delay_max,
                           uint32_t site_depth, uint32_t radius);

/* pxb_explore_row: candidate c of `parent`, materialised into out_row
 * (pxb_script_stride bytes; may be `parent` itself).  Host only, pure, never
 * touches the GPU; space->flag_mask and flags are not read.  PXB_E_INVAL for
 * c >= T, a changed keep site (nothing is written) and an invalid space.      */
int pxb_explore_row(const pxb_config* cfg, uint32_t depth, const pxb_explore_space* space,
                    const uint8_t* parent, uint64_t c, uint8_t* out_row);

/* pxb_explore_device: DEVICE buffers, asynchronous on `stream`, no device
 * synchronisation (everything is sized from count x T).  Runs the T candidates
 * of each of the `count` rows of d_rows (pxb_script_stride apart, 8-byte
 * aligned) and lists those that hold (space->flags & PXB_EXPLORE_MINIMAL: those
 * that are minimal) as g = (first_parent + i) T + c, ascending in g.  Cursor and
 * capacity as pxb_query_device's: *d_n_matches (required) is read as the write
 * cursor and then has the call's full count added; matches at or past
 * `capacity` are counted and not written, nothing at or past `capacity` entries
 * is touched, and d_ids may be NULL only when capacity == 0.
 *   d_counts (nullable)  count x 4 x 3 uint32, OVERWRITTEN: for each radius r in
 *                        0..3, {ran OK, held, minimal} ("ran OK": status OK and
 *                        within depth); 0 above `radius`.  The minimal column
 *                        is always computed; integer adds: bit-reproducible.
 *   d_status (nullable)  per parent PXB_TRACE_OK or PXB_SCRIPT_BAD; a bad parent
 *                        runs nothing, lists nothing and has zero counts, and
 *                        its neighbours are unaffected.
 * No candidate row is ever stored: a candidate is its parent's row read through
 * at most three (index, digit) pairs held in registers.  Scratch, from the
 * per-device stream-ordered pool on `stream`: 1 B per candidate + 12 B per 256.
 * PXB_E_INVAL, before any device call, for a null cfg, space or d_n_matches,
 * null rows with count > 0, depth > PXB_SCRIPT_MAX_DEPTH, site_depth 0 or >
 * depth, radius > 3, flag_mask & 0xFF == 0, unknown `flags` bits, T == 0,
 * count > 2^30, count x T > 2^32, rows not 8-byte aligned (ids and cursor 8,
 * counts and status 4), the d_ids rule above, and every config
 * pxb_trace_instance rejects.  count == 0 is valid.                            */
int pxb_explore_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                       const pxb_explore_space* space, uint64_t first_parent,
                       uint64_t* d_ids, uint64_t capacity, uint64_t* d_n_matches,
                       uint32_t* d_counts, uint32_t* d_status, void* stream);
/* pxb_explore: HOST buffers, blocking, on the current device; PXB_E_NODEV
 * without a GPU (checked after the validation above; count x T is not bounded
 * here).  *n_matches is OVERWRITTEN; first_parent is 0.  Walks the parents in
 * chunks of whole parents, at most PXB_EXPLORE_CHUNK candidates a chunk (a test
 * hook read like the others; default 2^26, clamped to [1, 2^32]) and at least
 * one parent, so device memory is one chunk's rows and flag bytes plus the
 * outputs (min(capacity, count x T) ids, the counts and the status).          */
int pxb_explore(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                const pxb_explore_space* space, uint64_t* ids, uint64_t capacity,
                uint64_t* n_matches, uint32_t* counts, uint32_t* status);

/* ---- coverage of an exploration (additive to ABI 5, found by symbol) -----------
 * Which handler classes lie within `radius` changed link entries of a row
 * (docs/SEMANTICS.md §15).  The space, its order, the sites, the alternatives,
 * the skipped candidates and a bad parent are pxb_explore's, unchanged:
 * pxb_explore_total and pxb_explore_row work on the ids this call lists.  A
 * candidate RAN OK as there (status PXB_TRACE_OK and no link consumed more than
 * `depth` entries); its MASK m is the coverage mask (PXB_COVER_*) of its run if
 * it ran OK and 0 otherwise.  It HOLDS when it ran OK, flag_mask == 0 or
 * result.flags & 0xFF & flag_mask != 0, and m matches the query q as in
 * pxb_cover_range: (m & all_mask) == all_mask, any_mask == 0 or m & any_mask
 * != 0, m & none_mask == 0.  With flag_mask != 0 and an all-zero q this is
 * pxb_explore's predicate.  MINIMAL is pxb_explore's rule over this predicate.
 * Per parent, one reach record of integer sums and minima (independent of the
 * launch order and of the host form's chunking).  Candidates are ordered by
 * radius, so the radius of first[b] is the reach distance of class b: the
 * smallest r with count[r][b] != 0.                                            */
typedef struct pxb_explore_reach {   /* 648 B, no implicit padding */
  uint32_t count[4][32];            /* [r][b]: candidates of radius r that ran OK and have class b; 0 above `radius` */
  uint32_t first[32];               /* the lowest candidate c (< T) with class b; 0xFFFFFFFF when none, and for b >= 29 */
  uint32_t parent_mask;             /* candidate 0's mask (0 if it did not run OK) */
  uint32_t union_mask;              /* the classes with any non-zero count */
} pxb_explore_reach;
typedef struct pxb_explore_cover_space {  /* 32 B */
  uint32_t site_depth;              /* 1..depth                                    */
  uint32_t radius;                  /* 0..PXB_EXPLORE_MAX_RADIUS                   */
  uint32_t flag_mask;               /* PXB_F_* bits of the predicate; 0: no outcome condition */
  uint32_t flags;                   /* PXB_EXPLORE_MINIMAL or 0                    */
  pxb_cover_query q;                /* reserved must be 0                          */
} pxb_explore_cover_space;

/* pxb_explore_cover_device: DEVICE buffers, asynchronous on `stream`, no device
 * synchronisation.  Ids, cursor, capacity, d_counts ({ran OK, held, minimal}
 * per radius) and d_status exactly as pxb_explore_device, with the predicate
 * above; d_reach (nullable, 8-byte aligned) takes `count` records, OVERWRITTEN;
 * a bad parent's record has zero counts and masks and an all-ones `first`.
 * Scratch as pxb_explore_device: 1 B per candidate + 12 B per 256.
 * PXB_E_INVAL for everything pxb_explore_device refuses except flag_mask == 0,
 * and for q.reserved != 0, a misaligned d_reach and PXB_CFG_TRACE_PRODUCTION.  */
int pxb_explore_cover_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                             const pxb_explore_cover_space* space, uint64_t first_parent,
                             uint64_t* d_ids, uint64_t capacity, uint64_t* d_n_matches,
                             uint32_t* d_counts, pxb_explore_reach* d_reach, uint32_t* d_status, void* stream);
/* pxb_explore_cover: HOST buffers, blocking, on the current device;
 * PXB_E_NODEV without a GPU (checked after the validation).  Chunked as
 * pxb_explore (whole parents per PXB_EXPLORE_CHUNK); no output depends on it.  */
int pxb_explore_cover(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                      const pxb_explore_cover_space* space, uint64_t* ids, uint64_t capacity,
                      uint64_t* n_matches, uint32_t* counts, pxb_explore_reach* reach, uint32_t* status);

/* ---- isolation windows as sites of the exploration (additive to ABI 5, found by symbol) ---
 * pxb_explore_cover over a larger space (docs/SEMANTICS.md §17): a candidate
 * changes at most `radius` link entries AND replaces the isolation window of at
 * most `win_radius` acceptors.  The LINK PART is pxb_explore's space unchanged
 * (S, A, T, the order, the digits, the skipped candidates, a bad parent); c is
 * one of its candidates, 0 <= c < T.  The WINDOW PART: with L = win_lens + (flags
 * & PXB_EXPLORE_WIN_OPEN ? 1 : 0) an acceptor has W = win_starts L alternatives;
 * digit d is start i = d / L and length index j = d % L: the window [c0, c1)
 * with c0 = win_first + i and c1 = c0 + 1 + j for j < win_lens, 4096 for the
 * open one.  With N = cfg->n_acceptors there are H = sum over q <= win_radius of
 * C(N, q) W^q WINDOW CHOICES, ordered as pxb_explore orders candidates over N
 * sites with W alternatives: by window radius, by the acceptors' combination
 * (a_1 < a_2, rank C(a_1, 1) + C(a_2, 2)), then by the digits, a_1's the least
 * significant.  Choice 0 leaves the parent's windows alone; a changed
 * acceptor's window REPLACES what the parent has there (explicit, none or the
 * 0xFFFF keep pair) and is never skipped.  CANDIDATE c' = h T + c, T_w = H T per
 * parent; its pair of radii is (r_w, r_l), its distance r_w + r_l.  Ran OK, the
 * mask and the predicate are pxb_explore_cover's.  A held candidate is MINIMAL
 * when no other candidate made of a subset of its window changes and a subset
 * of its link changes (same digits, the empty subsets included) holds.          */
#define PXB_EXPLORE_WIN_MAX_RADIUS 2u
#define PXB_EXPLORE_WIN_OPEN       2u   /* flags: one more length alternative, "to the end" (c1 = 4096) */
typedef struct pxb_explore_win_space {   /* 48 B, no implicit padding */
  uint32_t site_depth;              /* 1..depth                                    */
  uint32_t radius;                  /* 0..PXB_EXPLORE_MAX_RADIUS                   */
  uint32_t flag_mask;               /* PXB_F_* bits of the predicate; 0: no outcome condition */
  uint32_t flags;                   /* PXB_EXPLORE_MINIMAL | PXB_EXPLORE_WIN_OPEN  */
  pxb_cover_query q;                /* reserved must be 0                          */
  uint32_t win_radius;              /* 0..2 acceptors whose window a candidate replaces */
  uint32_t win_first;               /* first start step                            */
  uint32_t win_starts;              /* >= 1: starts win_first .. win_first + win_starts - 1 */
  uint32_t win_lens;                /* lengths 1..win_lens (may be 0 only with WIN_OPEN);
                                       win_first + win_starts - 1 + win_lens <= 4096 */
} pxb_explore_win_space;
typedef struct pxb_explore_win_reach {   /* 3080 B, no implicit padding */
  uint32_t count[3][4][32];         /* [r_w][r_l][b]: candidates of the cell that ran OK and have class b */
  uint32_t first[3][4][32];         /* the lowest c' (< T_w) of the cell with class b; 0xFFFFFFFF when none, and for b >= 29 */
  uint32_t parent_mask;             /* candidate 0's mask (0 if it did not run OK) */
  uint32_t union_mask;              /* the classes with any non-zero count */
} pxb_explore_win_reach;

/* T_w, or 0 for a space that is invalid or larger than 2^30 candidates
 * (flag_mask, q and PXB_EXPLORE_MINIMAL are not read).                        */
uint64_t pxb_explore_win_total(uint32_t n_proposers, uint32_t n_acceptors, uint32_t delay_max,
                               const pxb_explore_win_space* space);
/* pxb_explore_win_row: candidate c (c' above, < T_w) of `parent`, materialised
 * into out_row as pxb_explore_row does: the changed link bytes, and the
 * changed acceptors' windows as explicit (c0, c1) pairs.  Host only, pure.
 * PXB_E_INVAL for c >= T_w, a changed keep site of a link and an invalid space. */
int pxb_explore_win_row(const pxb_config* cfg, uint32_t depth, const pxb_explore_win_space* space,
                        const uint8_t* parent, uint64_t c, uint8_t* out_row);
/* pxb_explore_win_device: DEVICE buffers, asynchronous on `stream`, no device
 * synchronisation.  Ids (g = (first_parent + i) T_w + c', ascending), cursor,
 * capacity and d_status exactly as pxb_explore_cover_device.
 *   d_counts (nullable)  count x 3 x 4 x 3 uint32, OVERWRITTEN: [r_w][r_l]{ran OK,
 *                        held, minimal}.
 *   d_reach (nullable, 8-byte aligned)  `count` records, OVERWRITTEN; integer
 *                        adds and minima only: independent of the launch order
 *                        and of the host form's chunking.
 * No candidate row is ever stored.  Scratch as pxb_explore_device.  PXB_E_INVAL
 * for everything pxb_explore_cover_device refuses (with T_w in T's place and
 * PXB_EXPLORE_WIN_OPEN a known flag), and for win_starts == 0, win_radius > 2,
 * win_lens == 0 without WIN_OPEN, the 4096 bound above and T_w > 2^30.         */
int pxb_explore_win_device(const pxb_config* cfg, const uint8_t* d_rows, uint64_t count, uint32_t depth,
                           const pxb_explore_win_space* space, uint64_t first_parent,
                           uint64_t* d_ids, uint64_t capacity, uint64_t* d_n_matches,
                           uint32_t* d_counts, pxb_explore_win_reach* d_reach, uint32_t* d_status, void* stream);
/* pxb_explore_win: HOST buffers, blocking, on the current device; PXB_E_NODEV
 * without a GPU (checked after the validation).  Chunked as pxb_explore (whole
 * parents per PXB_EXPLORE_CHUNK); no output depends on it.                     */
int pxb_explore_win(const pxb_config* cfg, const uint8_t* rows, uint64_t count, uint32_t depth,
                    const pxb_explore_win_space* space, uint64_t* ids, uint64_t capacity,
                    uint64_t* n_matches, uint32_t* counts, pxb_explore_win_reach* reach, uint32_t* status);

/* ---- shrinking over a coverage predicate (additive to ABI 5, found by symbol) ---
 * pxb_shrink_batch with one change, the PREDICATE of a run (docs/SEMANTICS.md
 * §16): status PXB_TRACE_OK; flag_mask == 0 or result.flags & 0xFF & flag_mask
 * != 0; the run's coverage mask m (PXB_COVER_*, as pxb_cover gives it) matches q
 * as in pxb_cover_range ((m & all_mask) == all_mask, any_mask == 0 or m &
 * any_mask != 0, m & none_mask == 0); and no link consumed more than `depth`
 * entries.  With flag_mask & 0xFF != 0 and an all-zero q it is pxb_shrink_batch;
 * flag_mask == 0 with an all-zero q is "ran OK within depth", which the benign
 * schedule holds, so every such row shrinks to no faults.  Faults, neutralising,
 * the settling, the rounds, the budget, the statuses, the signature, the
 * in-place shrink in a scratch copy written back at the end, the nullable
 * outputs, one stream synchronisation per launch and the independence of a
 * row's outputs from its batch are pxb_shrink_batch's, unchanged.  One output
 * more:
 *   d_masks      uint32 (nullable): the coverage mask of the returned row's
 *                accepted run; NOT_INPUT / TOO_MANY: the given row's mask as
 *                pxb_cover gives it (0 when its status is not PXB_TRACE_OK),
 *                beside d_results, which is the given row's as well.
 * Scratch is pxb_shrink_batch's plus 4 B per row and, in the initial and prefix
 * launches, 4 B per candidate.  PXB_E_INVAL, before any device call, for
 * everything pxb_shrink_batch refuses except flag_mask & 0xFF == 0, and for a
 * null pred, flag_mask & ~0xFF, a non-zero reserved word of pred or q, mask bits
 * at or above PXB_COVER_CLASSES in q, a misaligned d_masks and
 * PXB_CFG_TRACE_PRODUCTION.                                                   */
typedef struct pxb_shrink_pred {   /* 32 B */
  uint32_t flag_mask;               /* PXB_F_* bits; 0: no outcome condition       */
  uint32_t max_launches;            /* >= 1                                        */
  uint32_t reserved[2];             /* must be 0                                   */
  pxb_cover_query q;                /* reserved must be 0                          */
} pxb_shrink_pred;
int pxb_shrink_cover_batch_device(const pxb_config* cfg, uint8_t* d_rows, uint64_t count, uint32_t depth,
                                  const pxb_shrink_pred* pred,
                                  uint32_t* d_status, uint32_t* d_n_faults, uint32_t* d_launches,
                                  uint16_t* d_sent, pxb_result* d_results, uint64_t* d_signature,
                                  uint32_t* d_masks, void* stream);
/* pxb_shrink_cover_batch: HOST buffers, blocking, on the current device;
 * PXB_E_NODEV without a GPU (checked after the validation above).  ids
 * non-null: rows is output only, as pxb_shrink_batch.                         */
int pxb_shrink_cover_batch(const pxb_config* cfg, const uint64_t* ids, uint8_t* rows, uint64_t count, uint32_t depth,
                           const pxb_shrink_pred* pred,
                           uint32_t* status, uint32_t* n_faults, uint32_t* launches,
                           uint16_t* sent, pxb_result* results, uint64_t* signature, uint32_t* masks);

/* ---- misc ----------------------------------------------------------------- */
const char* pxb_strerror(int code);
int         pxb_last_hip_error(void);
int         pxb_abi_version(void);
/* canonical algorithmic bytes for a fault-free P = 1 instance */
uint64_t    pxb_canonical_bytes_nofault(uint32_t n_acceptors);

#ifdef __cplusplus
}
#endif
#endif /* PAXOS_BATCH_H */
