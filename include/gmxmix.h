/* gmxmix.h -- C ABI of libgmxmix.so: gmix's mixer hot path on AMD MI355X (gfx950).
 *
 * This is the drop-in boundary for ONE path of byronknoll/gmix: the per-bit mixer (the 33
 * `Mixer` objects that `Predictor::AddMixers` builds and that `Predictor::Predict()` /
 * `Perceive()` / `Learn()` run after the feature models).  Everything else in gmix -- the
 * context models, the arithmetic coder, the CLI -- stays on the host and is not part of this
 * library.  Citations are file:line in the reference tree (/root/reference).
 *
 * Object model
 *   gmx_group : S independent mixer banks ("streams") of one topology on one device.  One
 *               bank = everything the last 33 entries of Predictor::models_ own: the
 *               LongTermMemory::mixers tables (long-term-memory.h:27-40) plus each Mixer's
 *               steps_/max_steps_/contexts_seen_ (mixer.h:33-38).  S = 1 is the drop-in for a
 *               single Predictor; S > 1 is the embarrassingly parallel multi-file case.
 *   gmx_batch : pinned host staging + device buffers for up to max_bits bits of per-stream
 *               records {predictions[N], active mask, contexts[M], bit} and the results.
 *
 * Conventions
 *   - every function returns 0 (GMX_OK) or a negative gmx_status; nothing throws or aborts
 *     across this boundary (the reference's Model methods are void and never fail,
 *     model.h:22-37; HIP failures are mapped to GMX_ERR_HIP and the text kept for
 *     gmx_last_error()).
 *   - a group is bound to one HIP stream and is not thread-safe (the reference Predictor is
 *     single-threaded and not re-entrant); distinct groups are independent.
 *   - results are a pure function of (bank state, inputs): the batched and the per-bit entry
 *     points produce identical floats (the encoder/decoder symmetry the reference's tester
 *     relies on, tester.cpp:350-356).
 *   - arithmetic parity: every mixer output, probability, weight and counter equals what the
 *     reference's strict C++ build computes, bit for bit (fp32 left-to-right sums, separate
 *     multiply and add roundings, IEEE divide, glibc's expf restated in gmx_math.h).
 */
#ifndef GMXMIX_H_
#define GMXMIX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gmx_status {
  GMX_OK = 0,
  GMX_ERR_INVALID = -1,      /* bad argument / unsupported topology */
  GMX_ERR_NOMEM = -2,        /* host or device allocation failed */
  GMX_ERR_HIP = -3,          /* a HIP runtime call failed; see gmx_last_error() */
  GMX_ERR_NO_DEVICE = -4,    /* no usable gfx950 device: there is no CPU fallback */
  GMX_ERR_STATE = -5,        /* call order violated (e.g. learn without forward) */
  GMX_ERR_FORMAT = -6        /* malformed checkpoint bytes on import */
} gmx_status;

/* One Mixer constructor call (mixer.h:17-19; the literals of predictor.cpp:251-358):
 * layer 0/1/2, gate-table size (rows), learning rate (the reference narrows a double
 * literal to float at the call).  The gate context itself is per-bit data. */
typedef struct gmx_mixer_desc {
  int32_t layer;
  uint32_t table_size;
  float learning_rate;
} gmx_mixer_desc;

/* What Predictor's constructor fixes before AddMixers runs (predictor.cpp:17-40):
 * num_predictions, models_with_skip_connection (lstm-model.cpp:12-14) and the mixers in
 * construction order: all layer-0 mixers, then layer-1, then at most one final mixer.
 * Limits: n_mixers <= 64, n_skip <= 8, n_inputs <= 2048,
 * layer-1 and final rows <= 64 weights. */
typedef struct gmx_topology {
  int32_t n_inputs;
  int32_t n_skip;
  const int32_t* skip_index;     /* [n_skip] indices into predictions */
  int32_t n_mixers;
  const gmx_mixer_desc* mixers;  /* [n_mixers] */
} gmx_topology;

typedef struct gmx_group gmx_group;
typedef struct gmx_batch gmx_batch;

/* ---- library ------------------------------------------------------------------------ */
const char* gmx_strerror(int status);
const char* gmx_last_error(void);          /* text of the last GMX_ERR_HIP on this thread */
int gmx_device_count(int* count);          /* gfx950 devices visible */
const char* gmx_build_info(void);          /* arch, flags, version */
/* PCI address of a device ("0000:c1:00.0", len >= 13): the key of /sys/bus/pci/devices/<id>/numa_node, so that
 * the host threads feeding a device (the reference's feature models, one Predictor per stream) can be kept on
 * the cores next to it. */
int gmx_device_pci_bus_id(int device, char* buf, size_t len);

/* ---- group: replaces Predictor::AddMixers' 33 objects (predictor.cpp:251-358) ---------- */
int gmx_group_create(gmx_group** out, const gmx_topology* topo, int n_streams, int device);
void gmx_group_destroy(gmx_group* g);
int gmx_group_n_streams(const gmx_group* g);
int gmx_group_n_mixers(const gmx_group* g);
int gmx_group_n_inputs(const gmx_group* g);
uint64_t gmx_group_bank_bytes(const gmx_group* g);   /* device bytes per stream */
int gmx_group_reset(gmx_group* g);                   /* all banks back to the constructed state */
int gmx_group_sync(gmx_group* g);                    /* wait for everything queued on its stream */
/* HIP events on the group's stream: start is recorded behind what is queued so far, stop behind
 * what was queued since; *ms = device time between the two (stop waits for it). */
int gmx_group_timer_start(gmx_group* g);
int gmx_group_timer_stop(gmx_group* g, float* ms);

/* ---- per-bit surface: Predict / Perceive / Learn for one stream ------------------------ */
/* 33 x Mixer::Predict + the final squash of Predictor::Predict (mixer.cpp:51-106,
 * predictor.cpp:366-375).  predictions[n_inputs] is the raw ShortTermMemory::predictions
 * blackboard (stale slots allowed), active_models[n_active] the ascending model indices of
 * ShortTermMemory::active_models (NULL with n_active < 0 = every slot active), contexts[M]
 * the values of the context variables the mixers alias (mixer.h:31) read at call time.
 * *p_final receives the clamped probability; out_all (nullable) the M logit outputs
 * (mixer_layer0_outputs, mixer_layer1_outputs, final_mixer_output). Synchronous. */
int gmx_bank_forward(gmx_group* g, int stream, const float* predictions,
                     const int32_t* active_models, int n_active, const uint32_t* contexts,
                     float* p_final, float* out_all);
/* Predictor::Perceive(bit) + 33 x Mixer::Learn (predictor.cpp:378-387, mixer.cpp:108-176)
 * on the inputs latched by the preceding gmx_bank_forward of that stream.  Optional, like
 * Learn() in the reference (generation never calls it, runner-utils.cpp:199-209). */
int gmx_bank_learn(gmx_group* g, int stream, int bit);

/* ---- batched surface: T bits for every stream in one launch ---------------------------- */
#define GMX_BATCH_OUTPUTS 1u   /* also return all M mixer outputs per bit */
#define GMX_BATCH_MASK 2u      /* records carry an active mask; otherwise every slot is active */
#define GMX_BATCH_LAST_OUTPUTS 8u  /* return the M outputs of each stream's LAST bit of a run only -- what the
                                    * blackboard (mixer_layer0_outputs, ..., final_mixer_output) holds afterwards; a
                                    * compressor needs no more, and the throughput build of the kernel then stores
                                    * nothing else beside the probabilities.  GMX_ERR_INVALID for the shapes that run
                                    * through the one-mixer and lane-pair kernels (use GMX_BATCH_OUTPUTS there), unless
                                    * gmx_group_set_register_rows would accept the group: its kernel keeps them. */
int gmx_batch_create(gmx_batch** out, gmx_group* g, uint64_t max_bits, unsigned flags);
void gmx_batch_destroy(gmx_batch* b);
/* Layout of the staging arrays (all stream-major, then bit):
 *   predictions [S][max_bits][n_pad]   n_pad = n_inputs rounded up to 4 (gmx_batch_n_pad)
 *   active_mask [S][max_bits][mask_words] bit i of word i/32 = model i is in active_models
 *   contexts    [S][max_bits][M]
 *   bits        [S][max_bits]
 *   p           [S][max_bits]          clamped probabilities (what Predict() returns)
 *   outputs     [S][max_bits][M]       with GMX_BATCH_OUTPUTS
 *   last_outputs[S][M]                 with GMX_BATCH_LAST_OUTPUTS */
int gmx_batch_n_pad(const gmx_batch* b);
int gmx_batch_mask_words(const gmx_batch* b);
uint64_t gmx_batch_max_bits(const gmx_batch* b);
float* gmx_batch_predictions(gmx_batch* b);     /* pinned host pointers, caller fills/reads */
uint32_t* gmx_batch_active_mask(gmx_batch* b);  /* NULL without GMX_BATCH_MASK */
uint32_t* gmx_batch_contexts(gmx_batch* b);
uint8_t* gmx_batch_bits(gmx_batch* b);
const float* gmx_batch_p(gmx_batch* b);
const float* gmx_batch_outputs(gmx_batch* b);   /* NULL without GMX_BATCH_OUTPUTS */
const float* gmx_batch_last_outputs(gmx_batch* b);  /* [S][M] after gmx_batch_download; NULL without GMX_BATCH_LAST_OUTPUTS */
/* Transfers run on streams of their own, ordered by events against the kernels that use the
 * batch: an upload starts when the last run of THIS batch is done and overlaps whatever runs on
 * other batches (double buffering: run(A); upload(B); run(B); download(A); wait(A); refill A ...);
 * everything queued on the group after gmx_batch_upload returns sees the new records.  A download
 * follows everything queued on the group so far -- except for a batch the host has already waited for
 * (gmx_batch_wait) with nothing queued on it since: that one is fetched at once, whatever the group's stream
 * holds by then.  A caller with several batches in flight fetches that way -- wait(A); download(A); wait(A) -- when
 * A's turn comes, rather than queueing download(A) right behind run(A): a copy that waits for its kernel holds up
 * the copies queued behind it, the uploads of the batches after it among them.  wait = this batch's upload, runs
 * and download.  (The same holds for gmx_ind_batch_* and gmx_lstm_batch_*.)
 * The batch's host arrays are read (upload) and written (download) when the copies execute, not when
 * the calls return: leave them alone between gmx_batch_upload / gmx_batch_download and the
 * gmx_batch_wait that follows. */
int gmx_batch_upload(gmx_batch* b, uint64_t n_bits);    /* async H2D of the first n_bits of every stream */
int gmx_batch_download(gmx_batch* b, uint64_t n_bits);  /* async D2H of p (and outputs) */
int gmx_batch_wait(gmx_batch* b);                       /* host waits for this batch's queued work */
/* Fill the DEVICE record buffers with the next n_bits of the synthetic stream of
 * BASELINE.json configs[1] (xorshift64; logits on the [-4,4] grid, 32-bit contexts, random
 * bits), generated on the GPU.  restart != 0 re-seeds stream s with
 * seed + s * 0x9E3779B97F4A7C15; restart == 0 continues where this batch's previous fill
 * stopped.  ctx_mode/ctx_mod/zero_mod/bit_mode as in oracle/gmx_synth.h. */
int gmx_batch_fill_synthetic(gmx_batch* b, uint64_t n_bits, uint64_t seed, uint64_t restart,
                             int ctx_mode, uint32_t ctx_mod, uint32_t zero_mod, int bit_mode);

/* Predict (+ Perceive + Learn when learn != 0) for bits [0, n_bits) of every stream from the
 * batch's device records; results land in the batch's device buffers.  Asynchronous on the
 * group's stream; kernel_ms (nullable) receives the kernel's duration measured with HIP
 * events on that stream, which makes the call synchronous. */
int gmx_group_run(gmx_group* g, gmx_batch* b, uint64_t n_bits, int learn, float* kernel_ms);

/* The same for streams that stand at different lengths -- S files compressed side by side
 * (runner-utils.cpp:43-67 once per file) end at different bits: stream s runs bits [0, n_bits[s]) of its
 * records, 0 = the stream sits this launch out.  The kernels with one stream per block (the reference's own shape and
 * the general kernel) take the counts as a per-block list: ONE launch whatever the lengths; the one-mixer and lane-pair
 * shapes, which put several streams into a wave, run one launch per stretch of neighbouring streams with equal counts
 * (GMX_RAGGED_SPLIT=1 in the environment forces that for every shape: a debugging aid).  The decay tables of the launch
 * are staged at a pitch of max(n_bits) for every stream.  Asynchronous on the group's stream. */
int gmx_group_run_ragged(gmx_group* g, gmx_batch* b, const uint64_t* n_bits /* [S] */, int learn);

/* ---- register-resident rows for any three-layer bank (opt-in) ---------------------------- */
/* By default only three literal shapes run with their rows in registers (one mixer; 90 or 256 inputs x 24/8/1);
 * every other topology takes the general kernel, which stages rows in LDS.  A bank whose AddMixers is not the
 * reference's can ask for the lane-pair kernel that serves the whole family: exactly three layers of 1..24 layer-0
 * mixers, 1..8 layer-1 mixers and a final mixer, exactly one skip input (at any index), 4..256 inputs, any table
 * sizes and learning rates.
 * gmx_topology_register_rows_eligible: 1 / 0 (host code only, no device needed); GMX_ERR_INVALID for a topology
 * gmx_group_create refuses.
 * gmx_group_set_register_rows: on != 0 sends gmx_group_run / gmx_group_run_ragged of this group (Predict, with or
 * without Learn; the 90- and 256-input shapes included) through that kernel, 0 back to the default routes; off when
 * a group is created.  GMX_ERR_INVALID, and nothing changes, when the topology is not eligible.  May be flipped
 * between launches: a bank's state in device memory is complete after every launch and its layout is the same for
 * every kernel.  Per-bit calls, lock step and chain steps are not affected.  Batches of such a group may be created
 * with GMX_BATCH_LAST_OUTPUTS whatever the switch says at that moment; ragged runs are ONE launch. */
int gmx_topology_register_rows_eligible(const gmx_topology* topo);
int gmx_group_set_register_rows(gmx_group* g, int on);

/* ---- persistence ------------------------------------------ */
/* Byte-compatible with the reference: *short_bytes = Mixer::WriteToDisk of every mixer in
 * order (3 x u64 each, mixer.cpp:178-182); *long_bytes = the mixer section of
 * LongTermMemory::WriteToDisk (long-term-memory.cpp:35-55).  Call with NULL buffers to size. */
int gmx_bank_export(gmx_group* g, int stream, void* long_buf, size_t* long_bytes,
                    void* short_buf, size_t* short_bytes);
int gmx_bank_import(gmx_group* g, int stream, const void* long_buf, size_t long_bytes,
                    const void* short_buf, size_t short_bytes);
/* Predictor::Copy for the mixer slice (mixer.cpp:190-195, long-term-memory.cpp:201-214). */
int gmx_bank_copy(gmx_group* dst, int dst_stream, gmx_group* src, int src_stream);
/* Checkpoint streams [first, first + count) of a group in one call; the learned rows are found and packed on the
 * device, so work and traffic follow the rows that exist, not the size of the banks.  Stream i's long section --
 * byte for byte what gmx_bank_export gives for it -- lies at long_buf + long_off[i], long_off[i + 1] - long_off[i]
 * bytes; its short section at short_buf + i * 24 * n_mixers.  long_off has count + 1 entries and is always filled.
 * With long_buf == NULL and short_buf == NULL the call only sizes (long_off[count] = bytes needed).
 * GMX_ERR_INVALID if long_cap < long_off[count]; nothing is written to long_buf then. */
int gmx_group_export(gmx_group* g, int first, int count, void* long_buf, size_t long_cap,
                     size_t* long_off /* [count + 1] */, void* short_buf /* [count][24 * n_mixers] */);
/* The inverse.  Every section is validated as gmx_bank_import validates it, and the rows of a mixer must ascend
 * strictly (GMX_ERR_FORMAT), BEFORE any bank is touched: a bad section anywhere leaves all banks as they were. */
int gmx_group_import(gmx_group* g, int first, int count, const void* long_buf,
                     const size_t* long_off /* [count + 1] */, const void* short_buf);
/* Mixer::GetMemoryUsage (mixer.cpp:197-205). */
int gmx_bank_memory_usage(gmx_group* g, int stream, int mixer, uint64_t* bytes);

/* ==== Lock-step surface: all S streams advance one bit per step ================================
 * S decoders on one GPU (coder/decoder.cpp:19-39: a decoder learns its bit from Predict's own
 * result) step together: Predict for all streams, S arithmetic decoders on the host, Learn for all
 * streams.  Each half -- and the pair learn + next predict -- is one hipGraph captured at creation (record uploads, the T = 1 kernel, the
 * download of the S probabilities), so a step costs two graph launches instead of a dozen runtime
 * calls.  Fill the host arrays of gmx_lockstep_batch (gmx_batch_predictions / _active_mask /
 * _contexts: one record per stream), call gmx_lockstep_predict, read gmx_batch_p (and
 * gmx_batch_outputs if created with GMX_BATCH_OUTPUTS), put the coded bits into gmx_batch_bits,
 * call gmx_lockstep_learn (asynchronous -- it works on a private copy of the bits, the array is the
 * caller's again when it returns; skip it for generation, runner-utils.cpp:199-209).
 * Same floats as every other surface.  Destroy before the group. */
/* GMX_LOCKSTEP_PERSISTENT (the reference's own mixer shape, up to 128 streams -- beyond, a graph's bulk copies
 * beat a thousand waves' small reads across the link): no graph launch and no stream synchronisation per step -- S persistent waves poll one doorbell,
 * fetch their records straight from the host arrays and write the probabilities straight back (the arrays
 * are read while gmx_lockstep_predict / _learn_predict run, never after they return).  Same calls, same
 * floats; where it does not apply the flag is ignored and the graphs are used. */
#define GMX_LOCKSTEP_PERSISTENT 4u
typedef struct gmx_lockstep gmx_lockstep;
int gmx_lockstep_create(gmx_lockstep** out, gmx_group* g, unsigned flags /* GMX_BATCH_OUTPUTS | GMX_LOCKSTEP_PERSISTENT */);
/* 1 if the object steps through persistent waves, 0 if through graphs */
int gmx_lockstep_is_persistent(const gmx_lockstep* ls);
void gmx_lockstep_destroy(gmx_lockstep* ls);
gmx_batch* gmx_lockstep_batch(gmx_lockstep* ls);
int gmx_lockstep_predict(gmx_lockstep* ls);
int gmx_lockstep_learn(gmx_lockstep* ls);
/* learn (bits in gmx_batch_bits) and the next predict (records in the host arrays) as one graph: the
 * step of S decoders once their first prediction is out.  Returns with the new probabilities. */
int gmx_lockstep_learn_predict(gmx_lockstep* ls);

/* ==== Indirect models =========================================
 * The producers of 82 of the mixers' 90 inputs: the reference's 41 `Indirect` objects
 * (models/indirect.h:11-34, constructed in predictor.cpp:78-120, :122-185, :210-250) and their
 * IndirectMemory (long-term-memory.h:11-25), for S streams on one device.  With a mixer batch
 * attached to gmx_indirect_run the predictions go from the models to the mixers inside HBM. */

/* One Indirect constructor call: table_size and learning_rate as in indirect.h:16-18; the two
 * prediction indices ShortTermMemory::AddPrediction returned for "<description>-indirect" and
 * "<description>-run_map" (indirect.cpp:10-13). */
typedef struct gmx_indirect_desc {
  uint32_t table_size;       /* the model owns 256 * table_size + 1 states (indirect.cpp:14-19) */
  float learning_rate;
  int32_t slot_indirect;
  int32_t slot_run_map;
} gmx_indirect_desc;

typedef struct gmx_indirect gmx_indirect;
typedef struct gmx_ind_batch gmx_ind_batch;

/* nonstationary_next / run_map_next: [256][2] next-state tables, state-major, of the two state
 * machines ShortTermMemory owns (short-term-memory.h `nonstationary`, `run_map`; the models call
 * their Next(state, bit), indirect.cpp:61-62, :67-68): fill them by calling Next() 512 times. */
int gmx_indirect_create(gmx_indirect** out, const gmx_indirect_desc* models, int n_models,
                        const uint8_t* nonstationary_next, const uint8_t* run_map_next,
                        int n_streams, int device);
void gmx_indirect_destroy(gmx_indirect* ib);
int gmx_indirect_n_streams(const gmx_indirect* ib);
int gmx_indirect_n_models(const gmx_indirect* ib);
uint64_t gmx_indirect_bank_bytes(const gmx_indirect* ib);   /* device bytes per stream */
int gmx_indirect_reset(gmx_indirect* ib);                   /* every table back to "never seen" */
int gmx_indirect_sync(gmx_indirect* ib);

/* Per-bit surface.  forward = n_models x Indirect::Predict (indirect.cpp:28-46): contexts[i] is
 * the value of model i's aliased context variable now, bit_context is
 * ShortTermMemory::bit_context; predictions[2*n_models] / active[2*n_models] (nullable) receive
 * what the blackboard slots of model i hold afterwards ([2i] indirect, [2i+1] run map: a model
 * that stays silent leaves its slot as it was) and whether SetLogitPrediction marked them
 * active (short-term-memory.cpp:193-197).  learn = n_models x Indirect::Learn
 * (indirect.cpp:48-69) with the contexts of the preceding forward.  Like gmx_bank_forward / gmx_bank_learn these
 * run through a persistent per-stream session (one mailbox command per bit, the learn travelling with the
 * next forward) where a session slot is free, else through a kernel launch per call; same floats. */
int gmx_indirect_forward(gmx_indirect* ib, int stream, const uint32_t* contexts, uint32_t bit_context,
                         float* predictions, uint8_t* active);
int gmx_indirect_learn(gmx_indirect* ib, int stream, int bit);

/* The Indirect models' Predict and the mixers' Predict of one bit as ONE call (predictor.cpp:366-368 runs them
 * back to back: the last feature models, then the 33 mixers): gmx_indirect_forward followed by gmx_bank_forward
 * with the models' predictions and active flags put into the mixers' inputs at slot_indirect / slot_run_map.
 * When both banks answer through per-bit sessions on the same device, the Indirect models' wave hands its
 * results to the mixers' wave itself: one host round trip instead of two.  `predictions` / `active_models`
 * (n_active >= 0) are the blackboard WITHOUT the Indirect models (their slots are overwritten, their indices
 * ignored); ind_predictions[2*n_models] / ind_active[2*n_models] (optional) return what gmx_indirect_forward
 * would.  Learn with gmx_indirect_learn and gmx_bank_learn as usual.  Same floats as the two calls. */
int gmx_chain_forward(gmx_indirect* ib, gmx_group* g, int stream, const uint32_t* ind_contexts,
                      uint32_t bit_context, const float* predictions, const int32_t* active_models, int n_active,
                      const uint32_t* contexts, float* p_final, float* out_all, float* ind_predictions,
                      uint8_t* ind_active);

/* Batched surface: records {contexts[n_models], bit_context, bit} of up to max_bits bits per
 * stream, results {predictions[2*n_models], active[2*n_models]} per bit. */
int gmx_ind_batch_create(gmx_ind_batch** out, gmx_indirect* ib, uint64_t max_bits);
void gmx_ind_batch_destroy(gmx_ind_batch* b);
uint64_t gmx_ind_batch_max_bits(const gmx_ind_batch* b);
uint32_t* gmx_ind_batch_contexts(gmx_ind_batch* b);       /* pinned host [S][max_bits][n_models] */
uint32_t* gmx_ind_batch_bit_contexts(gmx_ind_batch* b);   /* [S][max_bits] */
uint8_t* gmx_ind_batch_bits(gmx_ind_batch* b);            /* [S][max_bits] */
const float* gmx_ind_batch_predictions(gmx_ind_batch* b); /* [S][max_bits][2*n_models] */
const uint8_t* gmx_ind_batch_active(gmx_ind_batch* b);    /* [S][max_bits][2*n_models] */
int gmx_ind_batch_upload(gmx_ind_batch* b, uint64_t n_bits);
int gmx_ind_batch_download(gmx_ind_batch* b, uint64_t n_bits);
int gmx_ind_batch_wait(gmx_ind_batch* b);                  /* this batch's upload, runs, download (cf. gmx_batch_wait) */
/* Device-side generator of the synthetic stream of oracle/gmx_ind_synth.h (byte-structured
 * contexts, ctx_mod[4] moduli); stream s is seeded with seed + s * 0x9E3779B97F4A7C15. */
int gmx_ind_batch_fill_synthetic(gmx_ind_batch* b, uint64_t n_bits, uint64_t seed, uint64_t restart,
                                 const uint32_t* ctx_mod);
/* Predict (+ Learn when learn != 0) for bits [0, n_bits) of every stream.  `into` (nullable): a
 * batch of a mixer group with the same number of streams on the same device, created with
 * GMX_BATCH_MASK; the models' predictions are also written into its device prediction records
 * at their slot indices, their active bits replace those slots' bits of its mask records, and
 * the coded bits are copied into its bit records -- ordered after what was queued on the mixer
 * group before this call and before what is queued on it afterwards. */
int gmx_indirect_run(gmx_indirect* ib, gmx_ind_batch* b, uint64_t n_bits, int learn, gmx_batch* into,
                     float* kernel_ms);

/* ... for streams at different lengths (cf. gmx_group_run_ragged): stream s runs bits [0, n_bits[s]). */
int gmx_indirect_run_ragged(gmx_indirect* ib, gmx_ind_batch* b, const uint64_t* n_bits /* [S] */, int learn,
                            gmx_batch* into);

/* The indirect section of LongTermMemory::WriteToDisk / ReadFromDisk (long-term-memory.cpp:8-32,
 * :111-132), byte for byte; NULL buf to size.  Copy = long-term-memory.cpp:193-199;
 * memory_usage = Indirect::GetMemoryUsage (indirect.cpp:71-78). */
int gmx_indirect_export(gmx_indirect* ib, int stream, void* buf, size_t* bytes);
int gmx_indirect_import(gmx_indirect* ib, int stream, const void* buf, size_t bytes);
int gmx_indirect_copy(gmx_indirect* dst, int dst_stream, gmx_indirect* src, int src_stream);
int gmx_indirect_memory_usage(gmx_indirect* ib, int model, uint64_t* bytes);
/* Checkpoint streams [first, first + count) of an Indirect group in one call; live entries are found and packed on
 * the device.  Stream i's section -- byte for byte what gmx_indirect_export gives for it -- lies at
 * buf + off[i], off[i + 1] - off[i] bytes.  off has count + 1 entries and is always filled.  buf == NULL only sizes.
 * GMX_ERR_INVALID if cap < off[count]; nothing is written to buf then. */
int gmx_indirect_group_export(gmx_indirect* ib, int first, int count, void* buf, size_t cap,
                              size_t* off /* [count + 1] */);
/* The inverse.  Every section is validated as gmx_indirect_import validates it, and the keys of a sparse model must
 * ascend strictly (GMX_ERR_FORMAT), BEFORE any bank is touched: a bad section anywhere leaves all banks as they were. */
int gmx_indirect_group_import(gmx_indirect* ib, int first, int count, const void* buf,
                              const size_t* off /* [count + 1] */);

/* What the two blackboard slots of each model hold ([2i] indirect, [2i+1] run map): ShortTermMemory::predictions at
 * slot_indirect / slot_run_map, which the reference writes with the blackboard (short-term-memory.cpp:4) and which a
 * silent model leaves as they were (indirect.cpp:35-44).  The bank carries them through batches and chain calls, where
 * the host's copy goes stale (no mixer reads a silent slot, so only what is WRITTEN OUT depends on them): a caller that
 * takes a stream from the per-bit surface to the batched one sets them before and gets them after. */
int gmx_indirect_slots_get(gmx_indirect* ib, int stream, float* values /* [2 * n_models] */);
int gmx_indirect_slots_set(gmx_indirect* ib, int stream, const float* values /* [2 * n_models] */);

/* ==== LSTM byte model ==========================================
 * The reference's LstmModel (models/lstm-model.h:12-31): Lstm(256, 256, 50, 1, 100, 0.03, 10) over
 * the PPM byte distribution, predicting the next byte once per byte and the 8 bits from that
 * distribution; Lstm::Perceive learns the output layer every byte and runs back-propagation
 * through time + Adam over the last 100 bytes every 100th byte.  Batches are whole bytes. */
typedef struct gmx_lstm gmx_lstm;
typedef struct gmx_lstm_batch gmx_lstm_batch;

int gmx_lstm_create(gmx_lstm** out, int n_streams, int device);   /* constructed state, gate weights zero */
void gmx_lstm_destroy(gmx_lstm* l);
int gmx_lstm_n_streams(const gmx_lstm* l);
uint64_t gmx_lstm_bank_bytes(const gmx_lstm* l);
int gmx_lstm_reset(gmx_lstm* l);
int gmx_lstm_sync(gmx_lstm* l);
/* Gate weights in the reference's layout, LongTermMemory::neuron_layer_weights[3][50][563]
 * (forget gate, input node, output gate): what LstmLayer's constructor draws from rand()
 * (lstm-layer.cpp:179-194) or a checkpoint holds.  get also returns lstm_output_layer
 * [100][256][51] (nullable): together the LSTM section of LongTermMemory::WriteToDisk
 * (long-term-memory.cpp:57-68). */
int gmx_lstm_set_weights(gmx_lstm* l, int stream, const float* weights);
int gmx_lstm_get_weights(gmx_lstm* l, int stream, float* weights, float* output_layer);

/* Records per byte: ppm[256] = ShortTermMemory::ppm_predictions at the byte boundary
 * (mod_ppmd.cpp:1655-1661), the byte itself; results per bit: what LstmModel::Predict left in its
 * blackboard slot (SetPrediction: the logit; stale when the model stays silent) and whether it was
 * marked active; per byte: ShortTermMemory::lstm_prediction_context (lstm-model.cpp:25-33). */
int gmx_lstm_batch_create(gmx_lstm_batch** out, gmx_lstm* l, uint64_t max_bytes);
void gmx_lstm_batch_destroy(gmx_lstm_batch* b);
float* gmx_lstm_batch_ppm(gmx_lstm_batch* b);                  /* pinned host [S][max_bytes][256] */
uint8_t* gmx_lstm_batch_bytes(gmx_lstm_batch* b);              /* [S][max_bytes] */
const float* gmx_lstm_batch_predictions(gmx_lstm_batch* b);    /* [S][max_bytes][8] */
const uint8_t* gmx_lstm_batch_active(gmx_lstm_batch* b);       /* [S][max_bytes][8] */
const uint32_t* gmx_lstm_batch_contexts(gmx_lstm_batch* b);    /* [S][max_bytes] */
int gmx_lstm_batch_upload(gmx_lstm_batch* b, uint64_t n_bytes);
int gmx_lstm_batch_download(gmx_lstm_batch* b, uint64_t n_bytes);
int gmx_lstm_batch_wait(gmx_lstm_batch* b);                /* this batch's upload, runs, download (cf. gmx_batch_wait) */
/* LstmModel::Predict x 8 bits (+ LstmModel::Learn when learn != 0) for bytes [0, n_bytes) of every
 * stream. */
int gmx_lstm_run(gmx_lstm* l, gmx_lstm_batch* b, uint64_t n_bytes, int learn, float* kernel_ms);
/* ... for streams at different lengths (cf. gmx_group_run_ragged): stream s runs bytes [0, n_bytes[s]). */
int gmx_lstm_run_ragged(gmx_lstm* l, gmx_lstm_batch* b, const uint64_t* n_bytes /* [S] */, int learn);
/* Per-byte surface, for decoding (the byte is not known when its prediction is needed).
 * forward = Lstm::SetInput + Lstm::Predict(last_byte) at a byte boundary (lstm-model.cpp:19-33,
 * last_byte = ShortTermMemory::last_byte): probs[256]
 * (nullable) = the byte distribution LstmModel keeps in probs_, *context (nullable) =
 * lstm_prediction_context; the 8 bit predictions follow from probs and the decoded bits exactly as
 * in LstmModel::Predict (lstm-model.cpp:34-48).  perceive = Lstm::Perceive(byte), i.e.
 * LstmModel::Learn at the last bit of that byte. */
/* Hand a batch's results to the models downstream, device to device, after gmx_lstm_run:
 * mixer_batch (nullable; created with GMX_BATCH_MASK, max_bits >= 8 * n_bytes): the prediction of
 * bit k of byte n goes to slot `slot` (the LSTM's prediction index) of record 8n+k, its active
 * flag into that record's mask, lstm_prediction_context into gate-context column mixer_ctx_col
 * (< 0: none) of the 8 records; ind_batch (nullable): the context into column ind_ctx_col of the
 * 8 Indirect records (the model built on lstm_prediction_context, predictor.cpp:117-119). */
int gmx_lstm_feed(gmx_lstm* l, gmx_lstm_batch* b, uint64_t n_bytes, gmx_batch* mixer_batch, int slot,
                  int mixer_ctx_col, gmx_ind_batch* ind_batch, int ind_ctx_col);
int gmx_lstm_forward(gmx_lstm* l, int stream, int last_byte, const float* ppm, float* probs, uint32_t* context);
int gmx_lstm_perceive(gmx_lstm* l, int stream, int byte);

/* Persistence, byte for byte the reference's: `short` = the model's stretch of the .short file,
 * LstmModel::WriteToDisk / ReadFromDisk (lstm-model.cpp:62-76) with Lstm::, LstmLayer:: and 3 x
 * NeuronLayer::WriteToDisk behind it (lstm.cpp:124-158, lstm-layer.cpp:356-394, :62-122; 1 458 256
 * bytes); `long` = the LSTM section of LongTermMemory::WriteToDisk / ReadFromDisk
 * (long-term-memory.cpp:57-67, :151-160; 5 560 200 bytes).  Both buffers NULL: sizes only.  Where a byte has
 * ended top_/mid_/bot_ are written as the eighth LstmModel::Predict of the last coded byte leaves them.  Between
 * gmx_lstm_forward and gmx_lstm_perceive -- LstmModel::WriteToDisk works at any bit, and the reference's
 * TestGeneration checkpoints after a Predict whose byte is never perceived (tester.cpp:284, :312) -- the network's
 * state is what the forward left, and the range state, which the caller advances on the host from there
 * (lstm-model.cpp:34-48), is written as that forward's own Predict leaves it (255 / 127 / 0): a caller further into
 * the byte puts its own top_/mid_/bot_ into the first 12 bytes.  import takes either kind; a file does not say
 * whether its newest forward has been perceived (the reference keeps no such flag), so after an import of anything
 * but an untouched model both gmx_lstm_perceive and gmx_lstm_forward are accepted next.  After an import the
 * bank's remembered last byte is the newest perceived entry of input_history_; a stream that did not learn from its
 * last byte passes it explicitly (gmx_lstm_forward).
 * copy = LstmModel::Copy (lstm-model.cpp:78-85) + the LSTM share of LongTermMemory::Copy
 * (long-term-memory.cpp:216-219); memory_usage = LstmModel::GetMemoryUsage (lstm-model.cpp:87-101). */
int gmx_lstm_export(gmx_lstm* l, int stream, void* long_buf, size_t* long_bytes, void* short_buf,
                    size_t* short_bytes);
int gmx_lstm_import(gmx_lstm* l, int stream, const void* long_buf, size_t long_bytes, const void* short_buf,
                    size_t short_bytes);
int gmx_lstm_copy(gmx_lstm* dst, int dst_stream, gmx_lstm* src, int src_stream);
int gmx_lstm_memory_usage(gmx_lstm* l, uint64_t* bytes);
/* Many streams in one call: the group pair of include/gmxmix_lstm_group.h. */

/* ==== Match models ============================================================================
 * The producers of 6 of the mixers' 90 inputs and of the `longest_match` gate context: the reference's `Match`
 * objects (models/match.h:13-45, constructed in predictor.cpp:187-208), their MatchMemory and the deduplicated input
 * history (long-term-memory.h:42-53, :82), and the history rule of BasicContexts::Learn (basic-contexts.cpp:44-53),
 * for S streams on one device.  One bank owns the K models of a stream, its history and its longest_match; its inputs
 * are one context value per model and byte, and the coded bits. */

/* One Match constructor call (match.h:19-21): table_size, limit, and the prediction index
 * ShortTermMemory::AddPrediction returned (match.cpp:14-15). */
typedef struct gmx_match_desc {
  uint32_t table_size;
  int32_t limit;
  int32_t slot;
} gmx_match_desc;

typedef struct gmx_match gmx_match;
typedef struct gmx_match_batch gmx_match_batch;

/* n_models 1..8.  history_capacity: bytes of history a stream can hold (below 2^32; table entries are kept as u32).
 * Constructed state as match.cpp:3-23.  GMX_ERR_INVALID for bad arguments, GMX_ERR_NO_DEVICE without a GPU. */
int gmx_match_create(gmx_match** out, const gmx_match_desc* models, int n_models, uint64_t history_capacity,
                     int n_streams, int device);
void gmx_match_destroy(gmx_match* mb);
int gmx_match_n_streams(const gmx_match* mb);
int gmx_match_n_models(const gmx_match* mb);
uint64_t gmx_match_bank_bytes(const gmx_match* mb);   /* device bytes per stream, the history buffer included */
int gmx_match_reset(gmx_match* mb);                   /* every stream back to the constructed state */
int gmx_match_sync(gmx_match* mb);
int gmx_match_set_cu_mask(gmx_match* mb, const uint32_t* mask, int n_words);  /* cf. gmx_group_set_cu_mask */

/* Batched surface: records {contexts[K], bit_context, bit} of up to max_bits bits per stream, results
 * {predictions[K], active[K], longest_match} per bit.
 *   contexts     [S][max_bits][K]  model k's aliased context variable at Predict of that bit (it does not move within
 *                                  a byte); the kernel consumes the records of byte-opening bits (bit_context == 0)
 *                                  and the first record of a run
 *   bit_contexts [S][max_bits]     ShortTermMemory::bit_context, as in gmx_ind_batch
 *   bits         [S][max_bits]
 *   predictions  [S][max_bits][K]  what slot k of the blackboard holds after Predict (SetPrediction's logit; a model
 *                                  that stays silent, match_length_ <= 2, leaves it as it was)
 *   active       [S][max_bits][K]
 *   longest      [S][max_bits]     ShortTermMemory::longest_match after the K Predicts (match.cpp:70-73) */
int gmx_match_batch_create(gmx_match_batch** out, gmx_match* mb, uint64_t max_bits);
void gmx_match_batch_destroy(gmx_match_batch* b);
uint64_t gmx_match_batch_max_bits(const gmx_match_batch* b);
uint32_t* gmx_match_batch_contexts(gmx_match_batch* b);       /* pinned host pointers, caller fills / reads */
uint32_t* gmx_match_batch_bit_contexts(gmx_match_batch* b);
uint8_t* gmx_match_batch_bits(gmx_match_batch* b);
const float* gmx_match_batch_predictions(gmx_match_batch* b);
const uint8_t* gmx_match_batch_active(gmx_match_batch* b);
const uint32_t* gmx_match_batch_longest(gmx_match_batch* b);
int gmx_match_batch_upload(gmx_match_batch* b, uint64_t n_bits);
int gmx_match_batch_download(gmx_match_batch* b, uint64_t n_bits);
int gmx_match_batch_wait(gmx_match_batch* b);                  /* cf. gmx_batch_wait */
/* (Unlike the other banks' batches these transfers run on the bank's own stream, in order with its kernels: the bank
 * shares a stream priority level with the Indirect banks and adds one stream to it.) */
/* Predict AND Learn of bits [0, n_bits) of every stream, in Predictor's order (BasicContexts before the Match
 * objects in both loops): Match::Predict changes the models' state, so there is no predict-only batch.  A run may
 * begin and end anywhere in a byte.  `into` (nullable): a batch of a mixer group with the same number of streams on
 * the same device, created with GMX_BATCH_MASK; the predictions are also written into its device prediction records
 * at the models' slots, their active bits replace those slots' bits of its mask records, and longest_match is
 * written into each of the n_ctx_columns (<= 8) gate-context columns listed in ctx_columns (the reference's
 * topology: 6 and 30) -- ordered after what was queued on the mixer group before this call and before what is
 * queued on it afterwards, as for gmx_indirect_run.  The coded bits are NOT copied into the mixer batch:
 * gmx_indirect_run does that already.
 * Capacity: the library keeps an upper bound of every stream's history size (+1 per byte a run may complete).  When
 * a run could exceed history_capacity by that bound the true sizes are fetched from the device; if it still could,
 * the call returns GMX_ERR_INVALID before anything is queued. */
int gmx_match_run(gmx_match* mb, gmx_match_batch* b, uint64_t n_bits, gmx_batch* into, const int32_t* ctx_columns,
                  int n_ctx_columns, float* kernel_ms);
/* ... for streams at different lengths: stream s runs bits [0, n_bits[s]), 0 = it sits the launch out.  One launch. */
int gmx_match_run_ragged(gmx_match* mb, gmx_match_batch* b, const uint64_t* n_bits /* [S] */, gmx_batch* into,
                         const int32_t* ctx_columns, int n_ctx_columns);

/* Per-bit surface, a kernel launch per call.  forward = K x Match::Predict (match.cpp:25-74) with contexts[k] = model
 * k's aliased variable now; predictions[K] / active[K] / *longest_match (all nullable) as in the batch.  learn = the
 * history push of BasicContexts::Learn + K x Match::Learn (match.cpp:76-109) of the bit the preceding forward
 * predicted.  One forward per bit (GMX_ERR_STATE otherwise).  Same floats and the same state as the batched path;
 * the two may alternate on a stream between bits. */
int gmx_match_forward(gmx_match* mb, int stream, const uint32_t* contexts, uint32_t bit_context, float* predictions,
                      uint8_t* active, uint32_t* longest_match);
int gmx_match_learn(gmx_match* mb, int stream, int bit);

/* What the bank carries of ShortTermMemory besides longest_match: the K blackboard slots (cf.
 * gmx_indirect_slots_get) and new_bit, the last coded bit, which the next Match::Predict compares with the history
 * (match.cpp:29).  Both belong to the reference's ShortTermMemory checkpoint, not to Match's: gmx_match_import leaves
 * them alone, gmx_match_reset zeroes them, gmx_match_copy copies them.  A caller that restores a stream sets them
 * after the import.  get: values / new_bit nullable.  set also drops a pending gmx_match_forward of the stream: a bit
 * that is perceived but never learned (the reference's generation loop: Perceive -> Predict, no Learn) is handed over as
 * new_bit, and the next forward is its successor's -- no history push, no table entry, no count for the bit in between. */
int gmx_match_slots_get(gmx_match* mb, int stream, float* values /* [K] */, int* new_bit);
int gmx_match_slots_set(gmx_match* mb, int stream, const float* values /* [K] */, int new_bit);
int gmx_match_history_size(gmx_match* mb, int stream, uint64_t* size);   /* LongTermMemory::history.size() */

/* Byte for byte the reference's: `long` = the history and match section of LongTermMemory::WriteToDisk
 * (long-term-memory.cpp:70-106: u64 history size, the bytes, then per model u32 count of valid entries, {u32 key,
 * 5 pointer bytes} in ascending key order when count < 5/9 of the table, else 5 bytes per entry, 256 floats, 256
 * ints); `short` = Match::WriteToDisk of the K models in order (match.cpp:111-116, 11 bytes each).  Both buffers
 * NULL: sizes only.  Valid entries are counted and packed on the device.  import validates both sections before the
 * bank is touched -- lengths, the branch against the count, strictly ascending keys below the table size, every
 * pointer below the imported history size with a fifth byte of 0, the history size at most the capacity, bit_pos_ 0
 * or a power of two -- and returns GMX_ERR_FORMAT otherwise.  copy = Match::Copy and LongTermMemory::Copy's share, between
 * banks of the same models (table sizes, limits, slots) on the same device, GMX_ERR_INVALID otherwise;
 * memory_usage = Match::GetMemoryUsage (match.cpp:133-141). */
int gmx_match_export(gmx_match* mb, int stream, void* long_buf, size_t* long_bytes, void* short_buf,
                     size_t* short_bytes);
int gmx_match_import(gmx_match* mb, int stream, const void* long_buf, size_t long_bytes, const void* short_buf,
                     size_t short_bytes);
int gmx_match_copy(gmx_match* dst, int dst_stream, gmx_match* src, int src_stream);
int gmx_match_memory_usage(gmx_match* mb, int model, uint64_t* bytes);

/* Checkpoint streams [first, first + count) of a Match bank in one call; valid entries are counted and packed on the
 * device and every stream's section is assembled there.  Stream i's long section -- byte for byte what
 * gmx_match_export gives for it -- lies at long_buf + long_off[i], long_off[i + 1] - long_off[i] bytes; its short
 * section at short_buf + i * 11 * n_models.  long_off has count + 1 entries and is always filled.  long_buf == NULL
 * and short_buf == NULL: sizes only (exactly one of them NULL: GMX_ERR_INVALID).  GMX_ERR_INVALID if long_cap <
 * long_off[count]; nothing is written to long_buf or short_buf then.  count >= 1.  The sections are staged in one
 * device buffer of long_off[count] bytes that lives for the call: GMX_ERR_NOMEM, and nothing written, if it cannot be
 * had.  The number of launches, transfers and synchronisations of a call does not depend on count. */
int gmx_match_group_export(gmx_match* mb, int first, int count, void* long_buf, size_t long_cap,
                           size_t* long_off /* [count + 1] */, void* short_buf /* [count][11 * n_models] */);
/* The inverse (long_off[0] need not be 0).  Every section is validated as gmx_match_import validates it BEFORE any
 * bank is touched: a bad section anywhere (GMX_ERR_FORMAT) leaves all banks as they were.  Like gmx_match_import it
 * leaves the slot values and new_bit alone, and drops a pending gmx_match_forward of the imported streams. */
int gmx_match_group_import(gmx_match* mb, int first, int count, const void* long_buf,
                           const size_t* long_off /* [count + 1] */, const void* short_buf);

/* ==== Lock step through the whole device chain: S decoders, one device step per coded bit ======
 * The reference's Decoder (coder/decoder.cpp:19-39) learns each bit from Predict's own result, so S files being
 * restored on one GPU advance together, a bit per step (gmx_lockstep_* above does this for the mixers alone).  A
 * gmx_chainstep steps the LSTM byte model and the Indirect models with the mixers -- `ib` and `l` may be NULL: the
 * caller's records then carry those models' predictions like any other -- so that, as in the batched chain
 * (gmx_lstm_feed, gmx_indirect_run's `into`), the LSTM's prediction (slot lstm_slot of the mixers' inputs, its active
 * bit, lstm_prediction_context in gate-context column mixer_ctx_col and Indirect-context column ind_ctx_col; < 0: none)
 * and the Indirect models' 2 x K predictions never leave the device.
 * Per step the caller fills, for every stream s that takes part, what[s] and the host arrays the step reads:
 *   GMX_STEP_LEARN    bits[s] = the bit the stream decoded from the last step's p[s]: Predictor::Learn -- Mixer::Learn
 *                     x M, Indirect::Learn x K, and Lstm::Perceive when the bit completes a byte
 *   GMX_STEP_PREDICT  predictions[s][n_pad] (the blackboard; the device-side models' slots are overwritten), active_mask
 *                     [s][mask_words] (their bits left clear), contexts[s][M], ind_contexts[s][K], bit_contexts[s], and
 *                     -- when the bit opens a byte -- ppm[s][256] (ShortTermMemory::ppm_predictions): Predictor::Predict
 * and calls gmx_chainstep_step, which returns with p[s] (and outputs[s][M]) of the streams that predicted.  A stream
 * whose what[s] is 0 sits the step out (its file has ended) -- but not between a Predict and its Learn: the Learn belongs
 * to the very next step (GMX_ERR_STATE otherwise); streams start at a byte boundary.  One hipGraph of kernels per step;
 * same floats as every other surface.  Destroy before the banks.
 * gmx_chainstep_commit(cs, s), optional: stream s has filled what[s], bits[s] and its records for the coming step --
 * where the host can store into device memory the library moves them there right away, in the calling thread (S decoders
 * on several threads: each commits its own streams, any number of threads at once, before the one that calls
 * gmx_chainstep_step); streams nobody committed are moved by gmx_chainstep_step itself.  Nothing of stream s may be
 * written between its commit and the step.
 * gmx_chainstep_launch / gmx_chainstep_wait: gmx_chainstep_step in two halves -- launch returns with the step queued
 * (and `what` free to be cleared), wait with p / outputs in place -- for a caller that drives two objects alternately,
 * one's host work beside the other's device step.  Between the two, nothing of the object may be written or committed
 * (GMX_ERR_STATE). */
#define GMX_STEP_LEARN 1u
#define GMX_STEP_PREDICT 2u
typedef struct gmx_chainstep gmx_chainstep;
int gmx_chainstep_create(gmx_chainstep** out, gmx_group* g, gmx_indirect* ib /* nullable */, gmx_lstm* l /* nullable */,
                         int lstm_slot, int mixer_ctx_col, int ind_ctx_col);
void gmx_chainstep_destroy(gmx_chainstep* cs);
int gmx_chainstep_n_streams(const gmx_chainstep* cs);
float* gmx_chainstep_predictions(gmx_chainstep* cs);     /* pinned host [S][n_pad] */
uint32_t* gmx_chainstep_active_mask(gmx_chainstep* cs);  /* [S][mask_words] */
uint32_t* gmx_chainstep_contexts(gmx_chainstep* cs);     /* [S][M] */
uint32_t* gmx_chainstep_ind_contexts(gmx_chainstep* cs); /* [S][K]; NULL without Indirect models */
uint32_t* gmx_chainstep_bit_contexts(gmx_chainstep* cs); /* [S]; NULL without Indirect models and Match bank */
float* gmx_chainstep_ppm(gmx_chainstep* cs);             /* [S][256]; NULL without an LSTM */
uint8_t* gmx_chainstep_bits(gmx_chainstep* cs);          /* [S] */
uint8_t* gmx_chainstep_what(gmx_chainstep* cs);          /* [S] GMX_STEP_* */
const float* gmx_chainstep_p(gmx_chainstep* cs);         /* [S] */
const float* gmx_chainstep_outputs(gmx_chainstep* cs);   /* [S][M] */
int gmx_chainstep_commit(gmx_chainstep* cs, int stream);
int gmx_chainstep_step(gmx_chainstep* cs);
int gmx_chainstep_launch(gmx_chainstep* cs);
int gmx_chainstep_wait(gmx_chainstep* cs);
/* gmx_chainstep_attach_match: the Match models of every stream (a gmx_match bank of the same stream count on the same
 * device) step on the device as well: per step the history push of BasicContexts::Learn and K x Match::Learn, then
 * K x Match::Predict -- in idle lanes of the Indirect models' launch where there are Indirect models (at most 56) and a
 * mask of at most 8 words, in a launch of their own in front of the mixers' otherwise.  Their slots of predictions[s], their
 * bits of active_mask[s] (left clear by the caller) and longest_match in the gate-context columns ctx_columns[] (at most
 * 8) are the device's.  The caller fills bit_contexts[s] on every GMX_STEP_PREDICT and match_contexts[s][K] -- the
 * models' aliased context variables -- on predicts that open a byte (bit_contexts[s] == 0) and on a stream's first
 * predict through this object; streams need not start at a byte boundary.  Once, before the object's first step
 * (GMX_ERR_STATE otherwise); GMX_ERR_INVALID for another stream count or device, a model slot outside [0, n), a column
 * outside [0, M), more than 8 columns.  Nothing is kept outside the bank: between steps (and after the object is
 * destroyed) its streams may go on through gmx_match_run or gmx_match_forward / _learn, a pending gmx_match_forward
 * being dropped by a step as by a batch.  A step that could take a history past history_capacity returns
 * GMX_ERR_INVALID before anything is queued (the rule of gmx_match_run). */
int gmx_chainstep_attach_match(gmx_chainstep* cs, gmx_match* mb, const int32_t* ctx_columns, int n_ctx_columns);
uint32_t* gmx_chainstep_match_contexts(gmx_chainstep* cs);   /* pinned host [S][K_match]; NULL before attach */

/* ==== The Match models in the per-bit session chain ================================================
 * gmx_indirect_attach_match: the bank's streams ride in ib's per-bit session waves (lanes 56..63 of the one wave a
 * stream's Indirect models have; a process has no hardware queue for a fourth persistent kernel).  ctx_columns: the
 * mixers' gate-context columns that receive longest_match.  mb == NULL detaches.  GMX_ERR_INVALID: more than 56
 * Indirect models, another stream count or device, a column < 0, more than 8 columns, a Match slot that is also an
 * Indirect model's (a column beyond the mixer group's is refused by the call below, which knows the group).
 * GMX_ERR_STATE: mb is attached to a gmx_chainstep, or to another Indirect bank.  Attaching again replaces the
 * columns.  The two objects register with each other: destroying either one detaches first.
 *
 * gmx_chain_forward_match: gmx_match_forward, then gmx_chain_forward with the Match models' slot values and active
 * flags merged into predictions / active_models and contexts[ctx_columns[c]] = longest_match -- as ONE command and
 * one wait when gmx_chain_forward's own conditions for its one-round-trip path hold (same device, both banks on
 * sessions, mixers of the stock shape), as those calls one after the other otherwise: the same floats and the same
 * state in every bank either way.  Whatever the caller passes in the Match slots, the Indirect slots and those
 * columns is ignored.  Learn stays gmx_indirect_learn, gmx_bank_learn and gmx_match_learn; on a stream whose newest
 * Match forward went through a session wave gmx_match_learn only notes the bit, which travels with the stream's next
 * chained forward (every other gmx_match_* call that reads or writes the bank first stops ib's sessions and runs a
 * noted learn through the launch path; a learn that could take the history past history_capacity is refused by
 * gmx_match_learn itself, GMX_ERR_INVALID, and not noted).  Before either bank moves: GMX_ERR_INVALID for a column >=
 * the group's M or a Match slot >= its n; GMX_ERR_STATE for a second forward of the stream without a learn, and when
 * no bank is attached. */
int gmx_indirect_attach_match(gmx_indirect* ib, gmx_match* mb, const int32_t* ctx_columns, int n_ctx_columns);
int gmx_chain_forward_match(gmx_indirect* ib, gmx_group* g, int stream, const uint32_t* ind_contexts,
                            const uint32_t* match_contexts, uint32_t bit_context, const float* predictions,
                            const int32_t* active_models, int n_active, const uint32_t* contexts, float* p_final,
                            float* out_all, float* ind_predictions, uint8_t* ind_active,
                            float* match_predictions /* [K] */, uint8_t* match_active /* [K] */,
                            uint32_t* longest_match);

/* ==== Compute-unit shares ======================================================================
 * A bank's kernels normally spread over the whole chip.  Kernels of DIFFERENT banks that cannot share
 * a SIMD -- a mixer wave of the stock shape owns all 512 registers of its SIMD, an LSTM workgroup
 * half of every SIMD of its CU -- then run one after the other even from different streams.  With CU
 * masks (bit i of the 32-bit words = compute unit i; 8 words on MI355X, 32 CUs per XCD) the banks'
 * streams are re-created with hipExtStreamCreateWithCUMask and their kernels run side by side on
 * disjoint CUs: the LSTM on 16 CUs of every XCD, mixers and Indirect models on the other 16, is 24 %
 * faster end to end than all three on all CUs.  n_words == 0: all CUs again.  Call between launches
 * (the calls synchronise the bank); not with lock-step objects alive on a mixer group. */
int gmx_group_set_cu_mask(gmx_group* g, const uint32_t* mask, int n_words);
int gmx_indirect_set_cu_mask(gmx_indirect* ib, const uint32_t* mask, int n_words);
int gmx_lstm_set_cu_mask(gmx_lstm* l, const uint32_t* mask, int n_words);

/* ==== Context variables ========================================================================
 * The context values the models and mixers are gated by, computed on the device from the coded bits alone: the
 * context fields of BasicContexts (basic-contexts.cpp:5-40), IntervalContext (interval-context.cpp:3-23), SkipContext
 * (skip-context.cpp:9-18) and IndirectHash (indirect-hash.cpp:7-54) over ShortTermMemory's byte-level blackboard
 * (recent_bits, last_byte, rotating_history, recent_bytes), for S streams on one device.  A bank is described by an
 * ordered list of V <= 64 variables; a run writes, for every bit, the values the variables have at Predict of that
 * bit -- into a debugging array of the bank's own batch and into the context columns of up to three record batches
 * of the other banks.  In the lock-step chain the bank steps a bit at a time (gmx_chainstep_attach_ctx below), and so it
 * does on the per-bit surface (gmx_ctx_forward / gmx_ctx_learn) and in the per-bit session chain
 * (gmx_indirect_attach_ctx / gmx_chain_forward_ctx).  The adapter uses them in the opt-in *_dev builds (dropin/Makefile:
 * gmx::GpuCtxBank): every surface but the session chain. */
typedef enum gmx_ctx_kind {
  GMX_CTX_ZERO = 0,             /* always_zero */
  GMX_CTX_BIT_CONTEXT = 1,      /* bit_context = recent_bits - 1 */
  GMX_CTX_RECENT_BYTE = 2,      /* recent_bytes[index]; index 0 is last_byte.  index 0..9 */
  GMX_CTX_BYTE_PLUS_RECENT = 3, /* (recent_bytes[index] << 8) + bit_context.  index 0..9 */
  GMX_CTX_INTERVAL = 4,         /* IntervalContext(map, num_bits): num_bits 1..31, shift_ derived from map */
  GMX_CTX_SKIP = 5,             /* SkipContext(bytes_to_use): n_bytes 1..8 entries, each 0..15 */
  GMX_CTX_INDIRECT_HASH = 6     /* IndirectHash(outer_order, table_size, inner_order): orders 1..4 (the reference
                                 * shifts an int by 8 * (order - 1): larger orders are undefined there), table_size >= 1,
                                 * any size; at most 16 such variables per bank, each with a dense u32 table per
                                 * stream in device memory */
} gmx_ctx_kind;

typedef struct gmx_ctx_desc {
  int32_t kind;
  int32_t index;
  int32_t num_bits;
  int32_t n_bytes;
  int32_t outer_order, inner_order;
  uint32_t table_size;
  uint8_t bytes_to_use[8];
  uint8_t map[256];
} gmx_ctx_desc;

typedef struct gmx_ctx gmx_ctx;
typedef struct gmx_ctx_batch gmx_ctx_batch;

/* GMX_ERR_INVALID for bad arguments (V outside 1..64, more than 16 hash variables, a parameter outside the ranges
 * above, n_streams < 1), GMX_ERR_NO_DEVICE without a GPU: there is no CPU fallback.  Constructed state: every table
 * zero, the blackboard as ShortTermMemory's constructor leaves it, first_prediction_ set. */
int gmx_ctx_create(gmx_ctx** out, const gmx_ctx_desc* descs, int n_vars, int n_streams, int device);
void gmx_ctx_destroy(gmx_ctx* cb);
int gmx_ctx_n_streams(const gmx_ctx* cb);
int gmx_ctx_n_vars(const gmx_ctx* cb);
uint64_t gmx_ctx_bank_bytes(const gmx_ctx* cb);  /* device bytes per stream (stock: 201 MB, the nine hash tables) */
int gmx_ctx_reset(gmx_ctx* cb);
int gmx_ctx_sync(gmx_ctx* cb);
int gmx_ctx_set_cu_mask(gmx_ctx* cb, const uint32_t* mask, int n_words);  /* cf. gmx_group_set_cu_mask */

/* The bank's own batch: the coded bits of up to max_bits (<= 2^30) bits per stream, the only input.
 *   bits   [S][max_bits]      pinned host, caller fills
 *   values [S][max_bits][V]   pinned host, filled by download: every variable at Predict of every bit.  Only with
 *                             GMX_CTX_BATCH_VALUES; otherwise NULL, and no device array of that size exists.
 * Transfers run on the bank's own stream, like a Match batch's. */
#define GMX_CTX_BATCH_VALUES 1u
int gmx_ctx_batch_create(gmx_ctx_batch** out, gmx_ctx* cb, uint64_t max_bits, unsigned flags);
void gmx_ctx_batch_destroy(gmx_ctx_batch* b);
uint64_t gmx_ctx_batch_max_bits(const gmx_ctx_batch* b);
uint8_t* gmx_ctx_batch_bits(gmx_ctx_batch* b);
const uint32_t* gmx_ctx_batch_values(gmx_ctx_batch* b);
int gmx_ctx_batch_upload(gmx_ctx_batch* b, uint64_t n_bits);
int gmx_ctx_batch_download(gmx_ctx_batch* b, uint64_t n_bits);
int gmx_ctx_batch_wait(gmx_ctx_batch* b);

/* Where a run writes besides the batch's values.  Every member is nullable.  A route has one entry per context
 * column of the target's records (mixers: the group's M gate contexts; Indirect / Match: the bank's K models): the
 * index of the variable the column receives, or -1 to leave the column alone (longest_match is gmx_match_run's,
 * lstm_prediction_context gmx_lstm_feed's).  For the Indirect and the Match batch the run also writes the
 * bit_contexts and bits records; for the mixer batch only the routed columns (gmx_indirect_run copies the bits). */
typedef struct gmx_ctx_targets {
  gmx_batch* mixers;
  const int32_t* mixer_route;
  int32_t n_mixer_route;        /* == M */
  gmx_ind_batch* indirect;
  const int32_t* ind_route;
  int32_t n_ind_route;          /* == K of the Indirect bank */
  gmx_match_batch* match;
  const int32_t* match_route;
  int32_t n_match_route;        /* == K of the Match bank */
} gmx_ctx_targets;

/* Bits [0, n_bits) of every stream.  Record t holds the values at Predict of bit t, in Predictor's order
 * (BasicContexts first): byte-level variables move only at records where recent_bits == 1, and the very first Predict
 * of a stream is such a record (first_prediction_: BasicContexts returns early, every SkipContext, IntervalContext and
 * IndirectHash fires with last_byte 0 and an all-zero history).  A run may begin and end anywhere in a byte; the
 * stream's state in device memory is complete after every launch.  Writes into a target are ordered like
 * gmx_match_run's `into`: after what was queued on the target's owner before the call and after the target batch's
 * own upload, before what is queued on the owner afterwards.  Everything is validated before anything is queued:
 * GMX_ERR_INVALID for a target with another stream count or device, n_bits beyond a batch's max_bits, a route of the
 * wrong length (or longer than 128) or with an entry outside [-1, V). */
int gmx_ctx_run(gmx_ctx* cb, gmx_ctx_batch* b, uint64_t n_bits, const gmx_ctx_targets* targets, float* kernel_ms);
/* Of the newest gmx_ctx_run that was given kernel_ms: what the chain, the expand and the commit kernel took (ms[3];
 * their sum is that run's kernel_ms).  For scripts/bench_ctx.py. */
int gmx_ctx_last_kernel_ms(const gmx_ctx* cb, float* ms /* [3] */);
/* ... stream s runs bits [0, n_bits[s]), 0 = it sits the launch out.  One launch sequence whatever the lengths. */
int gmx_ctx_run_ragged(gmx_ctx* cb, gmx_ctx_batch* b, const uint64_t* n_bits /* [S] */,
                       const gmx_ctx_targets* targets);

/* What ShortTermMemory carries of this state (plus BasicContexts::first_prediction_ and the V current values), as
 * of the stream's newest Predict; new_bit is the bit coded since.  set refuses (GMX_ERR_INVALID) a blackboard whose
 * last_byte / recent_bytes are not what rotating_history holds at rotating_history_pos, recent_bits outside 1..255,
 * and first_prediction with recent_bits != 1.  A checkpoint taken inside a byte and restored into any stream of a
 * bank of the same variables continues identically (with gmx_ctx_import for the hash tables). */
typedef struct gmx_ctx_blackboard {
  int32_t recent_bits;
  int32_t new_bit;
  uint32_t last_byte;
  uint32_t rotating_history_pos;
  int32_t first_prediction;
  uint32_t recent_bytes[10];
  uint32_t values[64];
  uint8_t rotating_history[1000];
} gmx_ctx_blackboard;
int gmx_ctx_blackboard_get(gmx_ctx* cb, int stream, gmx_ctx_blackboard* out);
int gmx_ctx_blackboard_set(gmx_ctx* cb, int stream, const gmx_ctx_blackboard* in);

/* The concatenation, in descriptor order, of IndirectHash::WriteToDisk of the H hash variables, byte for byte
 * (indirect-hash.cpp:33-54): u32 count of non-zero entries; {u32 key, u32 value} in ascending key order when count <
 * table_size / 2 (integer division), else the whole table; u64 outer_context_, u32 outer_hash_.  offsets (nullable,
 * [H + 1]) receives where each variable's section begins.  buf == NULL: *bytes and offsets only.  Non-zero entries are
 * counted and packed on the device.  import validates everything before the bank is touched -- lengths, the branch
 * against the count, strictly ascending keys below the table size, no zero value in a sparse record, the count of a
 * dense one -- returns GMX_ERR_FORMAT otherwise, and leaves the blackboard alone. */
int gmx_ctx_export(gmx_ctx* cb, int stream, void* buf, size_t* bytes, size_t* offsets /* [H + 1] */);
int gmx_ctx_import(gmx_ctx* cb, int stream, const void* buf, size_t bytes);

/* Checkpoint streams [first, first + count) of a context bank in one call; non-zero entries are counted and packed on
 * the device and every stream's sections are assembled there.  Stream first + i's section -- byte for byte what
 * gmx_ctx_export gives for it -- lies at buf + off[i], off[i + 1] - off[i] bytes; off has count + 1 entries and is
 * always filled.  var_off (nullable, [count][H + 1]) receives where each variable's section begins inside its stream's
 * section (gmx_ctx_export's offsets).  buf == NULL: off and var_off only.  GMX_ERR_INVALID if cap < off[count]; nothing
 * is written to buf then.  count >= 1 and the window inside the bank, else GMX_ERR_INVALID.  A bank without hash
 * variables has empty sections: off all zero, nothing launched.  The sections pass through one device buffer and two
 * pinned host buffers in slices of consecutive streams that fit 64 MiB together (GMX_CKPT_STAGE_BYTES in the
 * environment, read at every call, replaces the cap; a slice is never less than one stream): the launches, transfers
 * and waits of a call depend on the number of slices, not on count. */
int gmx_ctx_group_export(gmx_ctx* cb, int first, int count, void* buf, size_t cap, size_t* off /* [count + 1] */,
                         size_t* var_off /* nullable [count][H + 1] */);
/* The inverse (off[0] need not be 0; the sections are contiguous).  Every section is validated as gmx_ctx_import
 * validates it BEFORE any bank is touched: a bad section anywhere (GMX_ERR_FORMAT) leaves all banks as they were.
 * Like gmx_ctx_import it leaves the blackboards alone. */
int gmx_ctx_group_import(gmx_ctx* cb, int first, int count, const void* buf, const size_t* off /* [count + 1] */);
/* count blackboards in one gather or scatter launch and one transfer, with the meaning of gmx_ctx_blackboard_get /
 * _set.  set validates all count boards before any is written: one bad board (GMX_ERR_INVALID) changes nothing.  On an
 * attached bank (gmx_chainstep_attach_ctx) get returns GMX_ERR_STATE and touches nothing if any stream of the window
 * stands between a Predict and its Learn; set clears that and makes the lock-step object read the boards again. */
int gmx_ctx_group_blackboard_get(gmx_ctx* cb, int first, int count, gmx_ctx_blackboard* out /* [count] */);
int gmx_ctx_group_blackboard_set(gmx_ctx* cb, int first, int count, const gmx_ctx_blackboard* in /* [count] */);
/* Debugging: launches, transfers and waits of the newest of the four calls above on this bank. */
int gmx_debug_ctx_group_ops(const gmx_ctx* cb);
/* Tables, hash states and blackboard of one stream into another, between banks of the same variables on the same
 * device.  (No entry point of this library locks: as everywhere, a handle is used by one thread at a time.) */
int gmx_ctx_copy(gmx_ctx* dst, int dst_stream, gmx_ctx* src, int src_stream);
/* GetMemoryUsage of the variable's object: IndirectHash 36 + 4 table_size (indirect-hash.cpp:83-89), IntervalContext
 * 256 * 4 + 8 + 4, SkipContext 4 n_bytes + 4; 0 for the fields of BasicContexts, which have no object of their own. */
int gmx_ctx_memory_usage(gmx_ctx* cb, int var, uint64_t* bytes);

/* ==== The context variables in the lock-step chain ==================================================
 * gmx_chainstep_attach_ctx: the context variables of every stream (a gmx_ctx bank of the same stream count on the same
 * device) step on the device as well, in one launch at the head of every step.  A route has the meaning
 * gmx_ctx_targets gives it: one entry per column, a variable index or -1 to leave the column alone -- to the caller, or
 * to another device-side writer (longest_match from the Match lanes, lstm_prediction_context from the LSTM lanes).
 * (A Match model reads its context word when a byte opens and keeps it for the byte, as before: a match_route names
 * byte-level variables, which the reference's Match contexts are.)
 * For every stream that takes part in a step:
 *   GMX_STEP_LEARN    the board's new_bit becomes bits[s]
 *   GMX_STEP_PREDICT  one record of gmx_ctx_run: new_bit is folded into recent_bits; when that completes a byte, or on
 *                     the stream's very first Predict, the ring takes the byte and every SKIP, INTERVAL and
 *                     INDIRECT_HASH variable fires; then the routed columns of contexts[s], ind_contexts[s] and
 *                     match_contexts[s], and bit_contexts[s] (with Indirect models or a Match bank), of this step's
 *                     device copy are written
 * After attach the staging arrays are ignored in the routed columns and in bit_contexts; unrouted columns keep the
 * caller's value.  bit_contexts, and a record array in which the caller owns no column, are no longer moved by
 * gmx_chainstep_commit or the step (gmx_chainstep_commit_bytes says what is).  Everything else about a step is
 * unchanged.  Nothing is kept outside the bank: after a step whose streams all ended on a Learn the board and the
 * tables are what gmx_ctx_run over the same bits leaves, and a stream may go on through either surface, from anywhere
 * in a byte (with an LSTM streams still start at a byte boundary).  The object reads every stream's position in its
 * byte from the board at attach and counts from there; after a gmx_ctx_run / _run_ragged, _blackboard_set, _copy or
 * _reset on the attached bank between steps it reads the boards again before its next step.  Between a stream's Predict and its Learn the board's new_bit means
 * nothing: gmx_ctx_run / _run_ragged with bits for that stream, gmx_ctx_blackboard_get and gmx_ctx_copy from it return
 * GMX_ERR_STATE and touch nothing; gmx_ctx_blackboard_set and gmx_ctx_reset clear that; gmx_ctx_export / _import touch
 * only the tables and stay allowed.
 * All of this is checked before anything is queued or changed.  GMX_ERR_STATE: not the object's first attach, a step
 * taken or in flight, the bank attached to another lock-step object; gmx_chainstep_attach_match after this call (a
 * Match bank is attached first) and gmx_ctx_set_cu_mask on an attached bank return it too.  GMX_ERR_INVALID: another
 * stream count or device; a route of the wrong length or longer than 128; an entry outside [-1, V); no mixer_route; an
 * ind_route without Indirect models or a match_route without an attached Match bank (and the reverse); a routed mixer
 * column that is one of the Match bank's ctx_columns or the object's mixer_ctx_col; a routed Indirect column equal to
 * ind_ctx_col.  The two objects register with each other: after the bank is destroyed the object's steps return
 * GMX_ERR_STATE. */
typedef struct gmx_ctx_step_routes {
  const int32_t* mixer_route;  int32_t n_mixer_route;   /* == M of the group; required */
  const int32_t* ind_route;    int32_t n_ind_route;     /* == K of the Indirect bank; NULL/0 iff the object has none */
  const int32_t* match_route;  int32_t n_match_route;   /* == K of the attached Match bank; NULL/0 iff none attached */
} gmx_ctx_step_routes;
int gmx_chainstep_attach_ctx(gmx_chainstep* cs, gmx_ctx* cb, const gmx_ctx_step_routes* routes);
/* Bytes of records per stream that gmx_chainstep_commit (or the step, for a stream nobody committed) moves to the
 * device as the object stands; 0 for NULL.  For scripts/bench_chainstep_ctx.py. */
uint64_t gmx_chainstep_commit_bytes(const gmx_chainstep* cs);
/* gmx_chainstep_step with HIP events recorded around the step's graph on the group's stream: *device_ms is what the
 * device spent on the step (0 when no stream asked for anything).  For scripts/bench_chainstep_ctx.py. */
int gmx_chainstep_timed_step(gmx_chainstep* cs, float* device_ms);

/* ==== The context variables one bit at a time ========================================================
 * gmx_ctx_forward is exactly one record of gmx_ctx_run for one stream: values ([V], nullable) receives every variable
 * at Predict of that bit, bit_context (nullable) ShortTermMemory::bit_context.  One launch and one wait.
 * gmx_ctx_learn makes `bit` the blackboard's new_bit -- what Predictor::Learn and Predictor::Perceive both leave for the
 * next BasicContexts::Predict, so a generated bit is perceived through the same call.  It is only noted and travels
 * with the stream's next forward; any other gmx_ctx_* call that reads or writes the stream runs a noted learn first.
 * A second forward of a stream without a learn in between returns GMX_ERR_STATE, and between a forward and its learn
 * the rules gmx_chainstep_attach_ctx gives for gmx_ctx_run / _run_ragged, _blackboard_get, _copy, _blackboard_set and
 * _reset hold unchanged.  A bank attached to a gmx_chainstep refuses both calls with GMX_ERR_STATE.  A stream may move
 * between this surface, gmx_ctx_run and the session chain below anywhere inside a byte. */
int gmx_ctx_learn(gmx_ctx* cb, int stream, int bit);
int gmx_ctx_forward(gmx_ctx* cb, int stream, uint32_t* values /* [V], nullable */, uint32_t* bit_context /* nullable */);

/* ==== The context variables in the per-bit session chain: the host sends one bit =======================
 * gmx_indirect_attach_ctx: the streams of `cb` (same stream count and device as ib) step in ib's per-bit session waves,
 * as a phase at the head of a chained forward.  routes has the meaning it has for gmx_chainstep_attach_ctx: mixer_route
 * is required, its length is checked against the group's M by the forward (GMX_ERR_INVALID there); ind_route is
 * required; match_route is given iff a Match bank is attached to ib already (attach the Match bank first:
 * gmx_indirect_attach_match on a bank with a context bank attached returns GMX_ERR_STATE); a routed mixer column must not
 * be one of the Match bank's ctx_columns.  cb == NULL detaches.  GMX_ERR_STATE: cb is attached to a gmx_chainstep or to
 * another Indirect bank; gmx_chainstep_attach_ctx on a bank that rides here returns it too.  The two objects register
 * with each other; destroying either detaches first.
 *
 * gmx_chain_forward_ctx: gmx_ctx_forward, then gmx_chain_forward_match (gmx_chain_forward when no Match bank is
 * attached to ib) with the routed columns of ind_contexts, match_contexts and contexts, and bit_context, taken from
 * the bank: the same floats and the same state in every bank as those calls one after the other.  ind_contexts /
 * match_contexts are read only in columns routed -1 and may be NULL when there is none; routed columns of `contexts`
 * are ignored.  ctx_values ([V]) and bit_context are outputs, nullable.  The learns are the usual calls
 * (gmx_ctx_learn, gmx_match_learn, gmx_indirect_learn, gmx_bank_learn): all are noted and travel with the next
 * forward.  Under gmx_chain_forward's own conditions for its one-round-trip path (same device, both banks on sessions,
 * stock-shape mixers, n_active >= 0, K <= 56 with a Match bank) the call is ONE command and ONE wait, and no context
 * word crosses the link; otherwise, or when no session slot is free, it is the launches one after the other.
 * Everything is validated before any bank moves.  GMX_ERR_STATE: nothing attached; a second forward of the stream
 * without gmx_ctx_learn (or, with a Match bank, without gmx_match_learn).  Every other gmx_ctx_* call that reads or
 * writes an attached bank (gmx_ctx_forward, the runs, the blackboards, copy, reset, export / import, the group calls)
 * first stops ib's sessions and runs a noted learn.  A wave restarted between a chained forward and its Indirect learn
 * recomputes the models' table indices from the blackboard's values, so whatever would move a stream's blackboard
 * outside its wave -- gmx_ctx_forward, the launch route of gmx_chain_forward_ctx, gmx_ctx_run / _run_ragged with bits
 * for the stream, gmx_ctx_blackboard_set, gmx_ctx_group_blackboard_set, gmx_ctx_copy into it, gmx_ctx_reset -- first
 * runs the Indirect learn noted for that forward.  When gmx_indirect_learn has not been called for it by then the
 * forward is void (a perceived bit's never is learned): a gmx_indirect_learn that comes afterwards returns
 * GMX_ERR_STATE and touches no table. */
int gmx_indirect_attach_ctx(gmx_indirect* ib, gmx_ctx* cb, const gmx_ctx_step_routes* routes);
int gmx_chain_forward_ctx(gmx_indirect* ib, gmx_group* g, int stream, const uint32_t* ind_contexts,
                          const uint32_t* match_contexts, const float* predictions, const int32_t* active_models,
                          int n_active, const uint32_t* contexts, float* p_final, float* out_all,
                          float* ind_predictions, uint8_t* ind_active, float* match_predictions,
                          uint8_t* match_active, uint32_t* longest_match, uint32_t* ctx_values, uint32_t* bit_context);

#ifdef __cplusplus
}
#endif
#endif /* GMXMIX_H_ */
