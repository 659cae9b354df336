/* ga3c_abi.h -- C ABI of libga3c_hip.so, the MI355X (gfx950) NetworkVP engine.
 *
 * This is the drop-in boundary for the reference's `Network` object
 * (/root/reference/ga3c, TensorFlow session calls).  Every entry point names the
 * reference interface it replaces.  Plain pointers and sizes only; no C++ types,
 * no exceptions cross this boundary.  All functions return 0 on success and a
 * negative GA3C_E* code on failure; ga3c_last_error() then holds a message for
 * the calling thread.
 *
 * Threading: one ga3c_net may be called concurrently from any number of host
 * threads (the reference calls predict from NP predictor threads and train from
 * NT trainer threads on one object without locks, Server.py:123-134,141-153).
 * Predictions run on per-call lanes; train steps are serialised; a prediction
 * sees either the weights before or after a train step, never a mix.
 */
#ifndef GA3C_ABI_H
#define GA3C_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GA3C_OK 0
#define GA3C_EINVAL (-1)   /* bad argument / shape */
#define GA3C_EHIP (-2)     /* HIP runtime error */
#define GA3C_ERCCL (-3)    /* RCCL error */
#define GA3C_ESTATE (-4)   /* call not valid in this state */
#define GA3C_ELOST (-5)    /* a row named by (agent, request number) is no longer in the state cache: the batch was not trained */

#define GA3C_FLAG_LOG_SOFTMAX 1u   /* Config.USE_LOG_SOFTMAX branch, NetworkVP_discrate.py:64-71 */
#define GA3C_FLAG_GRAD_CLIP 2u     /* Config.USE_GRAD_CLIP, tf.clip_by_average_norm, :120-123 */
#define GA3C_FLAG_DUAL_RMSPROP 4u  /* Config.DUAL_RMSPROP: one RMSProp optimizer per cost (cost_p, cost_v), :87-99,108-117,126-127;
                                      with GA3C_FLAG_GRAD_CLIP, tf.clip_by_norm per gradient tensor instead */
#define GA3C_FLAG_CONTINUOUS 8u    /* Config.CONTINUOUS_INPUT: the angle-output policy head of reference NetworkVP.py:92,95-105,175-204
                                      (DESIGN.md 8d).  p = atan2(sigmoid(d1 Wy + by) - 0.5, sigmoid(d1 Wx + bx) - 0.5) / pi is the
                                      action vector [B,A] (in (-1, 1]); a train batch's `a` is [B,A] float actions; every `z`
                                      output is [hx | hy], B x 2A (hx = d1 Wx + bx, hy = d1 Wy + by).  num_actions <= 32.
                                      With GA3C_FLAG_DUAL_RMSPROP: GA3C_EINVAL on ga3c_net (not supported yet); the
                                      vector-state network ga3c_mlp takes both */

#define GA3C_STATE_FLOATS 28224    /* 84*84*4 (Config.py:90-92) */
#define GA3C_MAX_ACTIONS 64

typedef struct ga3c_net ga3c_net;

/* Replaces the constructor arguments + Config reads of Network.__init__
 * (NetworkVP.py:37-46) and of the optimizer block (NetworkVP_discrate.py:99-105). */
typedef struct ga3c_net_config {
  int32_t device;          /* HIP device ordinal (Config.DEVICE 'gpu:N') */
  int32_t num_actions;     /* A */
  int32_t max_batch;       /* capacity in rows of one predict / train call */
  uint32_t flags;          /* GA3C_FLAG_* */
  float rmsprop_decay;     /* Config.RMSPROP_DECAY   (0.99) */
  float rmsprop_momentum;  /* Config.RMSPROP_MOMENTUM (0.0) */
  float rmsprop_epsilon;   /* Config.RMSPROP_EPSILON (0.1) */
  float log_epsilon;       /* Config.LOG_EPSILON     (1e-6) */
  float min_policy;        /* Config.MIN_POLICY      (0.0) */
  float grad_clip_norm;    /* Config.GRAD_CLIP_NORM  (40.0), used with GA3C_FLAG_GRAD_CLIP */
  int32_t predict_lanes;   /* concurrent prediction lanes (>=1; 0 -> 2) */
  int32_t train_lanes;     /* 0/1: synchronous train steps on one lane (default).  >= 2: Hogwild -- that many train
                              lanes update the weights in place from their own streams, concurrently and unlocked, as
                              the reference's NT trainer threads do (Server.py:132-134); not combinable with RCCL */
} ga3c_net_config;

const char* ga3c_last_error(void);
int ga3c_device_count(int32_t* count);
/* PCI address of a device ("0000:23:00.0", NUL-terminated into out[len]).  The host side places its threads and agent
 * processes on the cores next to that device (ga3c_amd/Placement.py); the reference leaves placement to TensorFlow's
 * `DEVICE` string alone (Config.py:62, NetworkVP.py:50). */
int ga3c_device_pci_bus_id(int32_t device, char* out, int32_t len);

/* Network.__init__ / session teardown.  Weights are zero until ga3c_net_set_arena(which = 0). */
int ga3c_net_create(const ga3c_net_config* cfg, ga3c_net** out);
int ga3c_net_destroy(ga3c_net* net);

/* Parameter arena.  Flat f32 in TensorFlow variable order and layout:
 * conv11/w[8,8,4,16] conv11/b[16] conv12/w[4,4,16,32] conv12/b[32] dense1/w[3872,256]
 * dense1/b[256] logits_v/w[256,1] logits_v/b[1] logits_p/w[256,A] logits_p/b[A].
 * GA3C_FLAG_CONTINUOUS: logits_p/{w,b} are replaced by logits_p/out_x/w[256,A] logits_p/out_x/b[A] logits_p/out_y/w[256,A]
 * logits_p/out_y/b[A] (TF creation order), OFF_WP + 2 (256 A + A) floats in all; names and checkpoints follow (12 variables).
 * Replaces get_variable_value / tf.train.Saver (NetworkVP.py:62-64,267-288).
 * which: 0 = weights, 1 = RMSProp `ms` slot, 2 = RMSProp `mom` slot, 3 = last gradient.
 * With GA3C_FLAG_DUAL_RMSPROP, 1 / 2 / 3 belong to the optimizer of cost_p (which stands in for cost_all) and
 * 4 = the value optimizer's `ms`, 5 = its `mom`, 6 = the last cost_v gradient; without the flag 4..6 are GA3C_EINVAL.
 * Slot regions the reference has no slot for (the value optimizer's on logits_p/{w,b}, the policy optimizer's on
 * logits_v/{w,b}) keep their initial values (ms = 1, mom = 0): no step writes them. */
int ga3c_net_param_count(ga3c_net* net, int64_t* count);
int ga3c_net_get_arena(ga3c_net* net, int32_t which, float* out, int64_t count);
int ga3c_net_set_arena(ga3c_net* net, int32_t which, const float* in, int64_t count);
int ga3c_net_get_step(ga3c_net* net, int64_t* step);        /* get_global_step, NetworkVP.py:233-235 */
int ga3c_net_set_step(ga3c_net* net, int64_t step);
/* The same variables BY NAME, for binders that do not want to re-derive the table above: get_variables_names /
 * get_variable_value (NetworkVP.py:284-288) and the name-keyed tf.train.Saver (NetworkVP.py:62-64).
 *   ga3c_net_num_params          10
 *   ga3c_net_param_name(i)       "conv11/w", "conv11/b", "conv12/w", "conv12/b", "dense1/w", "dense1/b", "logits_v/w",
 *                                "logits_v/b", "logits_p/w", "logits_p/b" (i in arena order; NULL outside [0, 10))
 *   ga3c_net_param_info          offset and element count of the variable inside the arena, its rank and shape (<= 4 dims)
 *   ga3c_net_get_param/set_param one variable of arena `which` (0 weights, 1 `ms`, 2 `mom`, 3 last gradient; set: 0..2;
 *                                GA3C_FLAG_DUAL_RMSPROP adds 4 / 5 / 6 as in ga3c_net_get_arena, set: 4..5);
 *                                `count` must equal the variable's element count.  A name may carry TensorFlow's ":0". */
int32_t ga3c_net_num_params(ga3c_net* net);
const char* ga3c_net_param_name(ga3c_net* net, int32_t index);
int ga3c_net_param_info(ga3c_net* net, const char* name, int64_t* offset, int64_t* count, int32_t* ndim, int64_t shape[4]);
int ga3c_net_get_param(ga3c_net* net, const char* name, int32_t which, float* out, int64_t count);
int ga3c_net_set_param(ga3c_net* net, const char* name, int32_t which, const float* in, int64_t count);
/* save / load (NetworkVP.py:267-282): the whole training state -- every variable, its two RMSProp slots and `step` -- in ONE
 * file.  The format is an uncompressed .npz (numpy.savez / numpy.load): members "<name>:0", "<name>/RMSProp:0",
 * "<name>/RMSProp_1:0" with the variable's shape, and "step" (int64 scalar); a TensorFlow checkpoint cannot be written
 * without TensorFlow.  The file name convention checkpoints/<model>_%08d (NetworkVP.py:267-272) is the caller's.  load refuses
 * a file whose shapes do not match this network (another action count) and leaves the network untouched then.
 * GA3C_FLAG_DUAL_RMSPROP: the slots are named as TF-1 would name two optimizers built value first (derived, not observed):
 * conv11/ conv12/ dense1/ variables carry the value optimizer's "/RMSProp:0" (ms) and "/RMSProp_1:0" (mom) and the policy
 * optimizer's "/RMSProp_2:0" and "/RMSProp_3:0"; logits_v/{w,b} the value optimizer's and logits_p/{w,b} the policy optimizer's
 * "/RMSProp:0" and "/RMSProp_1:0".  A dual network loads only such a file, a single-optimizer network only the other
 * kind (GA3C_ESTATE otherwise, network untouched). */
int ga3c_net_save(ga3c_net* net, const char* path);
int ga3c_net_load(ga3c_net* net, const char* path);

/* predict_p_and_v (NetworkVP.py:248-252): x f32[B,84,84,4] NHWC host buffer ->
 * p f32[B,A] (softmax_p), v f32[B] (logits_v); z f32[B,A] (logits_p) if not NULL.
 * GA3C_FLAG_CONTINUOUS: p is the action vector (the angle output) and z f32[B,2A] = [hx | hy] per row. */
int ga3c_net_predict(ga3c_net* net, const float* x, int32_t batch, float* p, float* v, float* z);
/* Same, states shipped as the uint8 frames of Environment._preprocess before its
 * `/128 - 1` (Environment.py:59-60); they stay uint8 in HBM and the conv kernels convert while
 * reading them, bit-identically to the f32 path. */
int ga3c_net_predict_u8(ga3c_net* net, const uint8_t* x, int32_t batch, float* p, float* v, float* z);

/* train (NetworkVP.py:254-257 = sess.run(train_op)): forward, loss, backward,
 * (all-reduce when a communicator is attached), RMSProp, global_step += 1.
 * y_r f32[B], a f32[B,A] one-hot (GA3C_FLAG_CONTINUOUS: the float action vectors taken).  losses (may be NULL) receives
 * {cost_p_1_agg, cost_p_2_agg, cost_v} (NetworkVP_discrate.py:61,83-84) of this rank's rows. */
int ga3c_net_train(ga3c_net* net, const float* x, const float* y_r, const float* a, int32_t batch,
                   float learning_rate, float beta, float* losses);
/* Same, states as uint8 frames (converted on the GPU exactly like ga3c_net_predict_u8). */
int ga3c_net_train_u8(ga3c_net* net, const uint8_t* x, const float* y_r, const float* a, int32_t batch,
                      float learning_rate, float beta, float* losses);
/* log (NetworkVP.py:259-265 = sess.run(summary_op) on the batch it is given): forward + loss of `batch` rows on the
 * current weights, no backward pass, no update, global_step unchanged.  The states come from exactly one of x (f32 host
 * buffer), x_u8 (uint8 frames) or offsets (rows in the registered segment, offsets_u8 as in ga3c_net_train_gather).
 * losses[3] = {cost_p_1_agg, cost_p_2_agg, cost_v}; d1 f32[B,256], v f32[B], p f32[B,A] (each may be NULL) receive the
 * activations the reference histograms (NetworkVP_discrate.py:143-146: denselayer, logits_v, softmax_p). */
int ga3c_net_evaluate(ga3c_net* net, const float* x, const uint8_t* x_u8, const int64_t* offsets, int32_t offsets_u8,
                      const float* y_r, const float* a, int32_t batch, float beta, float* losses, float* d1, float* v,
                      float* p);
/* The two halves of train, for tests and for callers that own the exchange step:
 * gradients only (left in arena 3), then the optimizer step on arena 3. */
int ga3c_net_compute_grads(ga3c_net* net, const float* x, const float* y_r, const float* a,
                           int32_t batch, float beta, float* losses);
int ga3c_net_apply_grads(ga3c_net* net, float learning_rate);

/* Device-resident path (inputs already in HBM; what bench.py times).
 * upload stages a batch into the train lane (y_r / a may be NULL for predict-only use). */
int ga3c_net_upload(ga3c_net* net, const float* x, const float* y_r, const float* a, int32_t batch);
int ga3c_net_upload_u8(ga3c_net* net, const uint8_t* x, const float* y_r, const float* a, int32_t batch);  /* same, uint8 frames */
int ga3c_net_predict_resident(ga3c_net* net, int32_t batch);   /* async on the train lane's stream */
int ga3c_net_train_resident(ga3c_net* net, int32_t batch, float learning_rate, float beta);
int ga3c_net_sync(ga3c_net* net);
/* Runs `iters` back-to-back resident steps (mode 0 = predict, 1 = train) between two HIP
 * events recorded on the stream the kernels run on; returns the elapsed milliseconds. */
int ga3c_net_time_resident(ga3c_net* net, int32_t mode, int32_t batch, int32_t iters,
                           float learning_rate, float beta, float* elapsed_ms);
/* `iters` resident prediction steps dealt round-robin over `nlanes` prediction lanes (the NP predictor threads of
 * Config.PREDICTORS, each with its own HIP stream); host wall-clock from first launch to all lanes drained. */
int ga3c_net_time_predict_lanes(ga3c_net* net, int32_t batch, int32_t iters, int32_t nlanes, float* elapsed_ms);
/* The block ga3c_net_time_predict_lanes timed last, as the GPU saw it: from the earliest lane's start event to the latest
 * lane's end event (milliseconds).  Unlike the host clock it does not contain the launch latency of the first kernel and
 * the wake-up of the waiting host threads, which at the driver's K = 20 are a tenth of a block. */
int ga3c_net_last_lanes_gpu_ms(ga3c_net* net, float* gpu_ms);
/* `iters` resident train steps dealt round-robin over `nlanes` train lanes of a net created with train_lanes >= 2
 * (nlanes = 1 works on any net); host wall-clock from the first launch to all lanes drained. */
int ga3c_net_time_train_lanes(ga3c_net* net, int32_t batch, int32_t iters, int32_t nlanes, float learning_rate,
                              float beta, float* elapsed_ms);
/* `iters` launches of ONE kernel of the image network's step on train lane 0, each between its own start / stop events; the
 * sum of the kernel times in milliseconds.  Every name is the step's own launcher of that kernel (grid, LDS, arguments and
 * whatever depends on `batch` alone are the step's) with the named variant forced at any batch, on the buffers the last step
 * left:
 *   forward   "conv_stack_fwd" (prediction form, f32 states), "conv_stack_fwd_train", "conv_stack_fwd_u8", "conv1_fwd",
 *             "conv1_fwd_u8", "conv2_fwd" (half grid), "conv2_fwd_q" (quarter grid), "dense1_fwd" (the step's choice, tile or
 *             fragment), "dense1_fwd_frag", "dense1_fwd_valu", "heads" (prediction form of the net's head)
 *   backward  "dense1_bwd_tile", "conv_bwd" (batch <= 128), "conv_bwd_wdstep" (with the deferred dense1/w step, lr = 0),
 *             "conv2_dw", "conv2_dx", "conv_dw_pair", "conv1_dw", "conv1_dw_u8", "slab_reduce" (the slabs the step of `batch`
 *             rows leaves), all without the fused update; "rmsprop" (no clip, no momentum, lr = 0)
 *   round 1   "dense1_dw", "dense1_dx", "dense1_bwd": kept for comparison, no step launches them; "dense1_dw" and
 *             "dense1_bwd" are GA3C_ESTATE on a GA3C_FLAG_CONTINUOUS net
 * "rmsprop" and "conv_bwd_wdstep" step in place with lr = 0: they advance the optimizer's `ms` ("conv_bwd_wdstep" on a net
 * with momentum also decays `mom` and moves dense1/w by it): use a scratch net.
 * An unknown name is GA3C_EINVAL. */
int ga3c_net_time_kernel(ga3c_net* net, const char* kernel, int32_t batch, int32_t iters,
                         float* elapsed_ms);

/* Activations / per-sample gradients of the last resident or train-lane step, for parity tests:
 * name in {"n1","n2","d1","z","p","v","dz","dv","dd1","dn2","dn1"}.  "dn1" is that of the last ga3c_net_compute_grads
 * (train steps of up to 128 rows consume it on chip and do not store it). */
int ga3c_net_fetch(ga3c_net* net, const char* name, float* out, int64_t count);
/* The same for prediction lane `lane` (name in {"z","p","v"}): the outputs of the last step that lane ran, e.g. the
 * resident steps of ga3c_net_time_predict_lanes, which leave them in HBM. */
int ga3c_net_fetch_lane(ga3c_net* net, int32_t lane, const char* name, float* out, int64_t count);

/* Zero-copy intake from the shared-memory transport (include/ga3c_host.h): register the whole segment
 * once (hipHostRegister), then a batch is described by one byte offset per row into that segment and the GPU
 * gathers the states itself (uint8 -> f32 fused) -- no host-side gather, no staging copy.  Offsets must be
 * 16-byte aligned; u8 != 0 means rows are 28,224 uint8 frames, else 28,224 f32.
 * Replaces the feed_dict copy of ThreadPredictor.py:57-58 / ThreadTrainer.py:52-59 + NetworkVP.py:252,257. */
int ga3c_net_register_host(ga3c_net* net, void* base, int64_t bytes);
int ga3c_net_unregister_host(ga3c_net* net);
int ga3c_net_predict_gather(ga3c_net* net, const int64_t* offsets, int32_t batch, int32_t u8, float* p, float* v,
                            float* z);
/* ga3c_net_predict_gather in two halves, for a predictor loop that answers the previous batch while the GPU works on this
 * one (ga3c_pq_serve_pipelined, include/ga3c_host.h): begin takes a lane, stages the offsets and ENQUEUES the step; end
 * waits for it, copies p[batch, A] and v[batch] out and gives the lane back.  Every begin must be followed by its end, from
 * the same thread (the lane stays taken in between); a thread may have two begun when the net has the lanes for it.  An end
 * for a ticket on which nothing is begun returns GA3C_ESTATE. */
int ga3c_net_predict_gather_begin(ga3c_net* net, const int64_t* offsets, int32_t batch, int32_t u8, int32_t* ticket);
int ga3c_net_predict_gather_end(ga3c_net* net, int32_t ticket, int32_t batch, float* p, float* v);
int ga3c_net_train_gather(ga3c_net* net, const int64_t* offsets, int32_t u8, const float* y_r, const float* a,
                          int32_t batch, float learning_rate, float beta, float* losses);

/* State cache (round 3): every state a trainer gathers out of the transport crossed PCIe once already, for its prediction --
 * and the gather's bursts on the bus are what training costs the predictions (profiles/README.md).  With a cache configured,
 * ga3c_net_predict_gather_begin_cached also keeps the uint8 state of every row it reads in HBM, in a ring of `depth`
 * states per agent: row i is named (agents[i], seqs[i]) -- the agent's id and the number of the request that carried the
 * state (ga3c_pq_request_seq, include/ga3c_host.h) -- and lands in slot seqs[i] % depth of its agent.  A train batch then
 * names its rows the same way (ProcessAgent.py:88-100 ships the state itself; NetworkVP.py:254-257 feeds it) and is
 * gathered HBM to HBM: ga3c_net_train_cached / ga3c_net_evaluate_cached = ga3c_net_train_gather / ga3c_net_evaluate on
 * those rows, bit for bit.  Every slot carries a tag, the request number it really holds, written once the step that stores
 * the state has been enqueued: a row whose slot holds another request (never stored, its step failed, or overwritten since)
 * or whose request is within 4 of falling out of its agent's window (a new prediction of that agent could overwrite it
 * before the copy has run) is refused with GA3C_ELOST and nothing is trained -- the caller drops the batch (ThreadTrainer
 * counts it).  `depth` is the caller's estimate of what an agent can have stored and not yet trained (Server.py: a multiple
 * of the agents' fair share of the rollouts in flight, not the worst case of one agent owning them all: 28,224 B per state,
 * 2.3 MB per agent at 80 states instead of 25 MB at 886); ga3c_net_stats reports the bytes held and the rows lost.  uint8
 * states, plain launches (no GA3C_GRAPHS: a replayed launch has its arguments baked in, the slots travel in them): up to 128
 * rows the conv stack stores the bytes it stages, beyond that the gathered batch is filed by a copy kernel behind the gather. */
int ga3c_net_state_cache_config(ga3c_net* net, int32_t max_agents, int32_t depth);
int ga3c_net_predict_gather_begin_cached(ga3c_net* net, const int64_t* offsets, const int32_t* agents, const int64_t* seqs,
                                         int32_t batch, int32_t u8, int32_t* ticket);
int ga3c_net_train_cached(ga3c_net* net, const int32_t* agents, const int64_t* seqs, const float* y_r, const float* a,
                          int32_t batch, float learning_rate, float beta, float* losses);
int ga3c_net_evaluate_cached(ga3c_net* net, const int32_t* agents, const int64_t* seqs, const float* y_r, const float* a,
                             int32_t batch, float beta, float* losses, float* d1, float* v, float* p);

/* Frame front-end on the device: Environment._rgb2gray + _preprocess
 * (ga3c/Environment.py:52-60) and the 4-deep frame queue of :62-74, so that an actor ships only the emulator's raw
 * RGB frame and the [84,84,4] state never leaves HBM.  The arithmetic is the reference's, bit for bit (see
 * include/ga3c_host.h: ga3c_frame_preprocess, and oracle/frame_frontend.py): f64 gray, per-frame min/max bytescale,
 * Pillow's BILINEAR resize to 84x84.
 *   frames_config     height x width x channels (3 or 4) of the frames to come; one queue per agent in [0,max_agents);
 *                     history > 0 also keeps the last `history` planes of every agent in HBM for train_frames
 *   frames_preprocess stateless: n frames -> n uint8 planes [84*84]                 (= Environment._preprocess)
 *   frames_push       n frames into the queues of n DISTINCT agents; reset[i] != 0 clears that queue first
 *                     (Environment.reset, :86-90)                                    (= _update_frame_q);
 *                     seq_out[i] (may be NULL) = sequence number of the plane agent i just got, counting from 0
 *   frames_push_offsets  the same for frames lying in the registered transport segment, one byte offset each: the
 *                     predictor hands over what it popped, nothing is copied on the host
 *   train_frames      one training step whose row i is the state agent[i]'s queue held right after its plane seq[i]
 *                     was pushed (planes seq-3 .. seq), re-assembled from the plane history -- rollouts then carry
 *                     (agent, seq, return, action) instead of 28,224-byte states (ProcessAgent.py:175 / ThreadTrainer.py:49-59)
 *   frames_state      one agent's uint8 [84,84,4] state and queue depth; depth < 4 means "no state yet" (:64-65)
 *   predict_frames    forward pass on the queued states of `agents` (every queue must be full)
 * rgb may be pageable, pinned, device memory or lie in the registered transport segment (read in place then). */
int ga3c_net_frames_config(ga3c_net* net, int32_t max_agents, int32_t height, int32_t width, int32_t channels,
                           int32_t history);
int ga3c_net_frames_preprocess(ga3c_net* net, const uint8_t* rgb, int32_t n, uint8_t* planes);
int ga3c_net_frames_push(ga3c_net* net, const uint8_t* rgb, const int32_t* agents, const uint8_t* reset, int32_t n,
                         int64_t* seq_out);
int ga3c_net_frames_push_offsets(ga3c_net* net, const int64_t* offsets, const int32_t* agents, const uint8_t* reset,
                                 int32_t n, int64_t* seq_out);
/* One predictor batch in raw-frame mode, one GPU round trip: the n popped requests' frames (byte offsets into the
 * registered segment) are pushed into their agents' queues -- flags[i] & 1: clear the queue first, flags[i] & 2: push
 * only (GA3C_REQ_RESET / GA3C_REQ_NO_PREDICT of include/ga3c_host.h) -- and rows i of p / v are filled for every request
 * that asked for a prediction.  This is the callback of the native predictor loop ga3c_pq_serve_frames. */
int ga3c_net_serve_frames(ga3c_net* net, const int64_t* offsets, const int32_t* agents, const uint32_t* flags, int32_t n,
                          float* p, float* v);
/* The same batch in two halves, for a loop that answers batch k while the GPU works on batch k + 1 (ga3c_pq_serve_frames_pipelined;
 * ThreadPredictor.py:45-66 is one loop: predict, then scatter): _begin pushes the frames and enqueues the forward pass, and
 * keeps the prediction lane it took (*ticket names it); _end (same n and flags) waits for the batch and fills p / v as
 * ga3c_net_serve_frames does.  Every _begin must be followed by its _end; ga3c_net_serve_frames is the two back to back. */
int ga3c_net_serve_frames_begin(ga3c_net* net, const int64_t* offsets, const int32_t* agents, const uint32_t* flags, int32_t n,
                                int32_t* ticket);
int ga3c_net_serve_frames_end(ga3c_net* net, int32_t ticket, const uint32_t* flags, int32_t n, float* p, float* v);
int ga3c_net_train_frames(ga3c_net* net, const int32_t* agents, const int64_t* seqs, const float* y_r, const float* a,
                          int32_t batch, float learning_rate, float beta, float* losses);
/* ga3c_net_evaluate for rows named by (agent, plane sequence number), as ga3c_net_train_frames takes them. */
int ga3c_net_evaluate_frames(ga3c_net* net, const int32_t* agents, const int64_t* seqs, const float* y_r, const float* a,
                             int32_t batch, float beta, float* losses, float* d1, float* v, float* p);
/* Planes pushed into `agent`'s queue so far = sequence number its next plane gets.  Server.add_agent hands it to an
 * agent process that takes over the id of a removed one, so that its rollouts keep naming planes the way the device
 * counts them. */
int ga3c_net_frames_pushed(ga3c_net* net, int32_t agent, int64_t* pushed);
int ga3c_net_frames_state(ga3c_net* net, int32_t agent, uint8_t* state, int32_t* filled);
int ga3c_net_predict_frames(ga3c_net* net, const int32_t* agents, int32_t n, float* p, float* v, float* z);
/* bench helpers: n frames resident in HBM, then `iters` pushes of them timed with events on the frames stream */
int ga3c_net_frames_upload(ga3c_net* net, const uint8_t* rgb, int32_t n);
int ga3c_net_time_frames(ga3c_net* net, int32_t n, int32_t iters, float* elapsed_ms);

/* Pinned host memory for staging arrays (ThreadPredictor.py:46-47 `states`), so that
 * predict/train copy by DMA without an intermediate host copy. */
int ga3c_host_alloc(void** ptr, int64_t bytes);
int ga3c_host_free(void* ptr);

/* Where the calls of a running engine spend their time (no counterpart in the reference; tools/e2e_probe.py and the
 * engine legs of bench.py print the deltas).  out[i] for i < n, i < GA3C_STAT_COUNT; times in nanoseconds since the
 * net was created (or since the last call with reset != 0). */
enum {
  GA3C_STAT_PREDICT_CALLS = 0,     /* prediction calls (predict, predict_gather, predict_frames, serve_frames) */
  GA3C_STAT_PREDICT_ROWS,          /* rows they carried */
  GA3C_STAT_PREDICT_LANE_WAIT_NS,  /* waiting for a free prediction lane */
  GA3C_STAT_PREDICT_LAUNCH_NS,     /* host time to enqueue a step */
  GA3C_STAT_PREDICT_SYNC_NS,       /* from the last launch to the lane's stream being idle (GPU time + queueing) */
  GA3C_STAT_PREDICT_WEIGHT_WAITS,  /* steps that had to wait on the GPU for an optimizer step in flight (theta_ready) */
  GA3C_STAT_TRAIN_CALLS,           /* train calls */
  GA3C_STAT_TRAIN_ROWS,
  GA3C_STAT_TRAIN_STAGE_NS,        /* staging a batch into an intake: offsets, gather launch, y / a copies (host time) */
  GA3C_STAT_TRAIN_LANE_WAIT_NS,    /* waiting for the train lane (another thread's step) with the batch already staged */
  GA3C_STAT_TRAIN_LAUNCH_NS,       /* host time to enqueue forward + backward + update */
  GA3C_STAT_TRAIN_SYNC_NS,         /* from the last launch to the step's completion */
  GA3C_STAT_TRAIN_READER_WAITS,    /* cross-stream waits a step issued for prediction lanes still reading the buffer it overwrites */
  GA3C_STAT_PREDICT_GPU_NS,        /* GPU span of a prediction step, first kernel's start to last kernel's end; collected only with
                                      GA3C_TIME_PREDICTIONS=1 in the environment (two timing events per step) */
  GA3C_STAT_STATE_CACHE_BYTES,     /* gauge: bytes of HBM the state cache holds (0: none configured) */
  GA3C_STAT_STATE_CACHE_LOST,      /* rows of train / evaluate batches that were refused with GA3C_ELOST */
  GA3C_STAT_COUNT
};
int ga3c_net_stats(ga3c_net* net, int64_t* out, int32_t n, int32_t reset);

/* Data-parallel training over RCCL (no counterpart in the reference, which is
 * single-device: Config.py:62).  id is an opaque 128-byte token made on rank 0 and
 * handed to every rank by the launcher.  After comm_init, train and apply_grads
 * all-reduce (sum) the gradient arena across ranks before the optimizer step. */
#define GA3C_COMM_ID_BYTES 128
int ga3c_comm_make_id(uint8_t id[GA3C_COMM_ID_BYTES]);
int ga3c_net_comm_init(ga3c_net* net, const uint8_t id[GA3C_COMM_ID_BYTES], int32_t rank, int32_t world);
/* What the attached communicator itself reports (ncclCommCount / ncclCommUserRank / ncclCommCuDevice), not what the
 * launcher's environment claims: ranks = 0 and rank = -1 while no communicator is attached.  bench.py's `rccl_ranks`. */
int ga3c_net_comm_info(ga3c_net* net, int32_t* ranks, int32_t* rank, int32_t* device);
/* `iters` back-to-back all-reduces of the gradient arena between two HIP events on the train stream (bench.py's
 * allreduce_us).  Collective: every rank of the communicator calls it. */
int ga3c_net_time_allreduce(ga3c_net* net, int32_t iters, float* elapsed_ms);
/* Sums the gradient arena (both halves, 2n floats, under GA3C_FLAG_DUAL_RMSPROP) over the ranks, on the train stream. */
int ga3c_net_allreduce_grads(ga3c_net* net);

/* ---- The vector-state network: reference NetworkVP.py:67-105,175-210, the network of GAME = 'Pendulum-v0' (DESIGN.md 8e).
 * x[B,S] -> dense11_p (4, linear) -> dense12_p (256, linear) -> dense13_p (256, linear) -> dense14_p (100, sigmoid)
 *        -> dense1 (64, sigmoid) -> logits_v (1) and the angle-output head logits_p/out_x, out_y (A each) of
 *        GA3C_FLAG_CONTINUOUS; loss, gradient, RMSProp and GA3C_FLAG_GRAD_CLIP as there.
 * A handle of its own: none of ga3c_net's workspace, lanes or fast paths apply.  Same conventions: int return codes,
 * ga3c_last_error(), arenas 0 weights / 1 `ms` / 2 `mom` / 3 last gradient.  One HIP stream carries every kernel of the
 * handle, so a prediction sees the weights before or after a train step, never a mix; train-type calls are serialised.
 * GA3C_FLAG_DUAL_RMSPROP: one optimizer per cost as on ga3c_net -- the trunk takes the value step and then the
 * policy step, logits_p/out_{x,y}/{w,b} only the policy optimizer's and logits_v/{w,b} only the value optimizer's; arenas 1 / 2 / 3 are the
 * policy optimizer's `ms` / `mom` / last cost_p gradient, 4 / 5 the value optimizer's `ms` / `mom`, 6 the last cost_v gradient
 * (exactly 0 where a cost has no path; slot regions without a slot keep ms = 1, mom = 0).  With GA3C_FLAG_GRAD_CLIP every
 * gradient tensor of both costs is clipped by tf.clip_by_norm instead.  The step still counts train calls.
 *
 * Arena (TF creation order, 16 variables, 4 S + 99,305 + 130 A floats): dense11_p/w[S,4] /b[4] dense12_p/w[4,256] /b[256]
 * dense13_p/w[256,256] /b[256] dense14_p/w[256,100] /b[100] dense1/w[100,64] /b[64] logits_v/w[64,1] /b[1]
 * logits_p/out_x/w[64,A] /b[A] logits_p/out_y/w[64,A] /b[A].
 * Checkpoints: the .npz container of ga3c_net_save with these 16 names; an image-network file and a vector-network file
 * each refuse to load into the other kind of network (GA3C_ESTATE, network untouched).  GA3C_FLAG_DUAL_RMSPROP names the slots
 * as ga3c_net_save does (derived, not observed): the trunk's variables carry the value optimizer's "/RMSProp:0", "/RMSProp_1:0"
 * (arenas 4, 5) and the policy optimizer's "/RMSProp_2:0", "/RMSProp_3:0" (arenas 1, 2); logits_v/{w,b} the value optimizer's
 * and logits_p/out_{x,y}/{w,b} the policy optimizer's "/RMSProp:0", "/RMSProp_1:0".  A dual network loads only such a file, a
 * single-optimizer network only the other kind (it tells a dual file by dense11_p/w/RMSProp_2:0): GA3C_ESTATE, untouched. */
typedef struct ga3c_mlp ga3c_mlp;
typedef struct ga3c_mlp_config {
  int32_t device;
  int32_t state_dim;       /* S, 1..64 (Pendulum: 3) */
  int32_t num_actions;     /* A, 1..32 (Pendulum: 1) */
  int32_t max_batch;       /* rows of one predict / train call */
  uint32_t flags;          /* GA3C_FLAG_CONTINUOUS (required) | GA3C_FLAG_GRAD_CLIP | GA3C_FLAG_DUAL_RMSPROP; anything else:
                              GA3C_EINVAL */
  float rmsprop_decay;
  float rmsprop_momentum;
  float rmsprop_epsilon;
  float grad_clip_norm;
  int32_t predict_lanes;   /* predictions in flight at once (begun and not ended); 0 -> 4 */
} ga3c_mlp_config;

int ga3c_mlp_create(const ga3c_mlp_config* cfg, ga3c_mlp** out);   /* weights zero until set_arena(0) */
int ga3c_mlp_destroy(ga3c_mlp* net);
int ga3c_mlp_param_count(ga3c_mlp* net, int64_t* count);
/* which: 0 weights, 1 `ms`, 2 `mom`, 3 last gradient; GA3C_FLAG_DUAL_RMSPROP adds 4 / 5 / 6 (above), GA3C_EINVAL without it.
 * get: any of them; set: 0..2 and, with the flag, 4..5 (a gradient arena is read only).  get_param / set_param alike. */
int ga3c_mlp_get_arena(ga3c_mlp* net, int32_t which, float* out, int64_t count);
int ga3c_mlp_set_arena(ga3c_mlp* net, int32_t which, const float* in, int64_t count);
int ga3c_mlp_get_step(ga3c_mlp* net, int64_t* step);
int ga3c_mlp_set_step(ga3c_mlp* net, int64_t step);
int32_t ga3c_mlp_num_params(ga3c_mlp* net);                         /* 16 */
const char* ga3c_mlp_param_name(ga3c_mlp* net, int32_t index);      /* arena order; NULL outside [0, 16) */
int ga3c_mlp_param_info(ga3c_mlp* net, const char* name, int64_t* offset, int64_t* count, int32_t* ndim, int64_t shape[4]);
int ga3c_mlp_get_param(ga3c_mlp* net, const char* name, int32_t which, float* out, int64_t count);
int ga3c_mlp_set_param(ga3c_mlp* net, const char* name, int32_t which, const float* in, int64_t count);
int ga3c_mlp_save(ga3c_mlp* net, const char* path);
int ga3c_mlp_load(ga3c_mlp* net, const char* path);
/* x f32[B,S] -> p f32[B,A] (the action vector), v f32[B]; z f32[B,2A] = [hx | hy] if not NULL. */
int ga3c_mlp_predict(ga3c_mlp* net, const float* x, int32_t batch, float* p, float* v, float* z);
/* One step: y_r f32[B], a f32[B,A] the actions taken; losses (may be NULL) = {cost_p_1_agg, cost_p_2_agg, cost_v}.
 * 2 launches (3 with GA3C_FLAG_GRAD_CLIP); the row sums run in row order: the same call gives the same bits. */
int ga3c_mlp_train(ga3c_mlp* net, const float* x, const float* y_r, const float* a, int32_t batch, float learning_rate,
                   float beta, float* losses);
int ga3c_mlp_compute_grads(ga3c_mlp* net, const float* x, const float* y_r, const float* a, int32_t batch, float beta,
                           float* losses);                                     /* gradient into arena 3, no update */
int ga3c_mlp_apply_grads(ga3c_mlp* net, float learning_rate);                 /* (clip +) RMSProp on arena 3 (dual: 6, then
                                                                                 3), step += 1 */
/* Forward + loss, no update: the states are x (host rows) or offsets (rows of the registered segment), exactly one.
 * pd1 f32[B,4], pd2 f32[B,256], d1 f32[B,64], v f32[B], p f32[B,A] (each may be NULL): what the reference's summary
 * histograms (NetworkVP.py:164-168) look at. */
int ga3c_mlp_evaluate(ga3c_mlp* net, const float* x, const int64_t* offsets, const float* y_r, const float* a, int32_t batch,
                      float beta, float* losses, float* pd1, float* pd2, float* d1, float* v, float* p);
/* Zero-copy intake: rows are S f32 (4 S bytes, 4-byte aligned, not 16) at byte offsets into the registered segment; u8 must
 * be 0.  predict_gather / _begin / _end have the signatures of ga3c_predict_rows_fn, ga3c_predict_begin_fn and
 * ga3c_predict_end_fn (include/ga3c_host.h), so the native predictor loops drive this network unchanged. */
int ga3c_mlp_register_host(ga3c_mlp* net, void* base, int64_t bytes);
int ga3c_mlp_unregister_host(ga3c_mlp* net);
int ga3c_mlp_predict_gather(void* net, const int64_t* offsets, int32_t batch, int32_t u8, float* p, float* v, float* z);
int ga3c_mlp_predict_gather_begin(void* net, const int64_t* offsets, int32_t batch, int32_t u8, int32_t* ticket);
int ga3c_mlp_predict_gather_end(void* net, int32_t ticket, int32_t batch, float* p, float* v);
int ga3c_mlp_train_gather(ga3c_mlp* net, const int64_t* offsets, int32_t u8, const float* y_r, const float* a, int32_t batch,
                          float learning_rate, float beta, float* losses);
/* Timing: upload stages a batch in HBM; time_resident runs `iters` steps on its first `batch` rows (mode 0 predict,
 * 1 train) between two events on the network's stream -> milliseconds. */
int ga3c_mlp_upload(ga3c_mlp* net, const float* x, const float* y_r, const float* a, int32_t batch);
int ga3c_mlp_time_resident(ga3c_mlp* net, int32_t mode, int32_t batch, int32_t iters, float learning_rate, float beta,
                           float* elapsed_ms);
/* Rows of the last train / compute_grads / evaluate / resident step, for tests: name in {"x", "pd1", "pd2", "pd3", "pd4",
 * "d1", "v", "z", "p", "dpd1", "dpd2", "dpd3", "dpd4", "dd1" (deltas at the layers' pre-activations), "dv", "dz",
 * "lossrow"}; count = rows x width.  GA3C_FLAG_DUAL_RMSPROP: "dd1", "dpd4" ... "dpd1" are cost_p's deltas and "dd1_v",
 * "dpd4_v" ... "dpd1_v" cost_v's (GA3C_EINVAL without the flag). */
int ga3c_mlp_fetch(ga3c_mlp* net, const char* name, float* out, int64_t count);

/* ---- The discrete-action vector-state network: reference NetworkVP_discrate.py:39-130, the network of GAME = 'CartPole-v0'
 * (DESIGN.md 8g).  x[B,S] -> dense1_<i>_p (w_i, sigmoid), i = 1..L -> logits_v (1) and logits_p (A) -> softmax; both loss
 * branches (GA3C_FLAG_LOG_SOFTMAX, min_policy, log_epsilon), gradient, RMSProp and GA3C_FLAG_GRAD_CLIP as there.
 *   chained = 0 (the reference, :52-56): every layer is [S, w_i] and reads x; only layer L reaches the heads.  Layers
 *     1..L-1 are variables that nothing reads: their gradient is exactly 0, and train / apply_grads / the clip pass leave
 *     their value, `ms` and `mom` untouched (TF-1 drops a variable whose gradient is None).  The reference's clip branch
 *     (:120-122) would raise on them; skipping them there too is this library's definition.
 *   chained = 1: layer i reads layer i - 1 ([w_{i-1}, w_i]); every variable is live.
 * A handle of its own with ga3c_mlp's conventions: int return codes, ga3c_last_error(), arenas 0 weights / 1 `ms` / 2 `mom`
 * / 3 last gradient, one HIP stream for every kernel and copy (a prediction sees the weights before or after a train step,
 * never a mix), a lane per prediction in flight, train-type calls serialised.
 *
 * Arena (TF creation order, 2 L + 4 variables): dense1_1_p/w /b ... dense1_L_p/w /b logits_v/w[w_L,1] /b[1]
 * logits_p/w[w_L,A] /b[A]; 4 x 50 + 11 + 11 A floats at S = 4 and the default widths (10, 10, 10, 10).
 * Checkpoints: the .npz container of ga3c_net_save with these names.  A file of another network kind, or of this kind with
 * a variable missing, of another shape, or with more layers, refuses to load (GA3C_ESTATE, network untouched); the file
 * carries variables, not the graph, so two wirings whose shapes coincide load into each other. */
#define GA3C_DMLP_MAX_LAYERS 8
typedef struct ga3c_dmlp ga3c_dmlp;
typedef struct ga3c_dmlp_config {
  int32_t device;
  int32_t state_dim;       /* S, 1..64 (CartPole: 4) */
  int32_t num_actions;     /* A, 1..32 (CartPole: 2) */
  int32_t max_batch;       /* rows of one predict / train call */
  int32_t num_layers;      /* L, 1..8 (Config.DENSE_LAYERS) */
  int32_t widths[GA3C_DMLP_MAX_LAYERS];   /* w_1..w_L, 1..256 each */
  int32_t chained;         /* 0: the reference's wiring; 1: layer i reads layer i - 1 */
  uint32_t flags;          /* GA3C_FLAG_LOG_SOFTMAX | GA3C_FLAG_GRAD_CLIP; anything else: GA3C_EINVAL */
  float rmsprop_decay;
  float rmsprop_momentum;
  float rmsprop_epsilon;
  float grad_clip_norm;
  float log_epsilon;
  float min_policy;
  int32_t predict_lanes;   /* predictions in flight at once (begun and not ended); 0 -> 4 */
} ga3c_dmlp_config;

int ga3c_dmlp_create(const ga3c_dmlp_config* cfg, ga3c_dmlp** out);   /* weights zero until set_arena(0) */
int ga3c_dmlp_destroy(ga3c_dmlp* net);
int ga3c_dmlp_param_count(ga3c_dmlp* net, int64_t* count);
int ga3c_dmlp_get_arena(ga3c_dmlp* net, int32_t which, float* out, int64_t count);      /* which 0..3 */
int ga3c_dmlp_set_arena(ga3c_dmlp* net, int32_t which, const float* in, int64_t count); /* which 0..2 */
int ga3c_dmlp_get_step(ga3c_dmlp* net, int64_t* step);
int ga3c_dmlp_set_step(ga3c_dmlp* net, int64_t step);
int32_t ga3c_dmlp_num_params(ga3c_dmlp* net);                         /* 2 L + 4 */
const char* ga3c_dmlp_param_name(ga3c_dmlp* net, int32_t index);      /* arena order; NULL outside [0, 2 L + 4) */
int ga3c_dmlp_param_info(ga3c_dmlp* net, const char* name, int64_t* offset, int64_t* count, int32_t* ndim, int64_t shape[4]);
int ga3c_dmlp_get_param(ga3c_dmlp* net, const char* name, int32_t which, float* out, int64_t count);
int ga3c_dmlp_set_param(ga3c_dmlp* net, const char* name, int32_t which, const float* in, int64_t count);
int ga3c_dmlp_save(ga3c_dmlp* net, const char* path);
int ga3c_dmlp_load(ga3c_dmlp* net, const char* path);
/* x f32[B,S] -> p f32[B,A] (the policy), v f32[B]; z f32[B,A] the logits if not NULL.  1 launch. */
int ga3c_dmlp_predict(ga3c_dmlp* net, const float* x, int32_t batch, float* p, float* v, float* z);
/* One step: y_r f32[B], a f32[B,A] one-hot rows of the actions taken; losses (may be NULL) = {cost_p_1_agg, cost_p_2_agg,
 * cost_v}.  2 launches (3 with GA3C_FLAG_GRAD_CLIP); the row sums run in row order: the same call gives the same bits. */
int ga3c_dmlp_train(ga3c_dmlp* net, const float* x, const float* y_r, const float* a, int32_t batch, float learning_rate,
                    float beta, float* losses);
int ga3c_dmlp_compute_grads(ga3c_dmlp* net, const float* x, const float* y_r, const float* a, int32_t batch, float beta,
                            float* losses);                                    /* gradient into arena 3, no update */
int ga3c_dmlp_apply_grads(ga3c_dmlp* net, float learning_rate);               /* (clip +) RMSProp on arena 3, step += 1 */
/* Forward + loss, no update (2 launches): the states are x (host rows) or offsets (rows of the registered segment), exactly
 * one.  lastdense f32[B,w_L], v f32[B], p f32[B,A] (each may be NULL): what the reference's summary histograms
 * (NetworkVP_discrate.py:143-146) look at. */
int ga3c_dmlp_evaluate(ga3c_dmlp* net, const float* x, const int64_t* offsets, const float* y_r, const float* a, int32_t batch,
                       float beta, float* losses, float* lastdense, float* v, float* p);
/* Zero-copy intake, as ga3c_mlp_*: rows are S f32 at 4-byte aligned byte offsets into the registered segment; u8 must be 0.
 * predict_gather / _begin / _end have the signatures of ga3c_predict_rows_fn, ga3c_predict_begin_fn and ga3c_predict_end_fn
 * (include/ga3c_host.h), so the native predictor loops drive this network unchanged. */
int ga3c_dmlp_register_host(ga3c_dmlp* net, void* base, int64_t bytes);
int ga3c_dmlp_unregister_host(ga3c_dmlp* net);
int ga3c_dmlp_predict_gather(void* net, const int64_t* offsets, int32_t batch, int32_t u8, float* p, float* v, float* z);
int ga3c_dmlp_predict_gather_begin(void* net, const int64_t* offsets, int32_t batch, int32_t u8, int32_t* ticket);
int ga3c_dmlp_predict_gather_end(void* net, int32_t ticket, int32_t batch, float* p, float* v);
int ga3c_dmlp_train_gather(ga3c_dmlp* net, const int64_t* offsets, int32_t u8, const float* y_r, const float* a, int32_t batch,
                           float learning_rate, float beta, float* losses);
/* Timing: upload stages a batch in HBM; time_resident runs `iters` steps on its first `batch` rows (mode 0 predict,
 * 1 train) between two events on the network's stream -> milliseconds. */
int ga3c_dmlp_upload(ga3c_dmlp* net, const float* x, const float* y_r, const float* a, int32_t batch);
int ga3c_dmlp_time_resident(ga3c_dmlp* net, int32_t mode, int32_t batch, int32_t iters, float learning_rate, float beta,
                            float* elapsed_ms);
/* Rows of the last train / compute_grads / evaluate / resident step, for tests: name in {"x", "h<i>" (output of layer
 * i = 1..L), "dh<i>" (the delta at its pre-activation), "v", "z", "p", "dv", "dz", "lossrow"}; count = rows x width.  A layer
 * nothing reads has neither rows nor a name here (GA3C_EINVAL). */
int ga3c_dmlp_fetch(ga3c_dmlp* net, const char* name, float* out, int64_t count);

/* ---- Device actors (Config.DEVICE_AGENTS): n CartPole-v0 environments, their rollouts and their training rows
 * in HBM, stepped by this handle on its one stream between its own predict and train kernels.  What a step does is
 * ProcessAgent.run_episode / run over EnvironmentCart.Environment with RETURN_MODE = 'fork' (DISCOUNTING, no intermediate
 * rewards): action 0 without a prediction on an environment's first ever step; the one-draw action of ga3c_select_action;
 * f64 physics; reward r * 0.005 - 1; a rollout cut on done or time_count == time_max with its last row kept as row 0 of the
 * next one; the returns of ga3c_returns_fork in f64, cast to f32; a reset that leaves the observation alone.  The uniforms
 * are u(seed, environment, draw number) = (mix(mix(seed + G (environment + 1)) + G (draw + 1)) >> 11) 2^-53 with splitmix64's
 * finalizer mix and G = 0x9E3779B97F4A7C15, all sums mod 2^64; an action takes one draw, a reset four (create
 * stands for the host's two resets before the first step: draws 0..3 are passed over, 4..7 are the first physics).
 * create: the network must have S = 4 and A = 2 and n (time_max + 1) <= max_batch (GA3C_EINVAL); a second create is
 * GA3C_ESTATE, as is every other call here without actors.  destroy: also done by ga3c_dmlp_destroy. */
#define GA3C_ACTORS_MAX_STEPS 64
int ga3c_dmlp_actors_create(ga3c_dmlp* net, int32_t n, int32_t time_max, double discount, int64_t seed);
int ga3c_dmlp_actors_destroy(ga3c_dmlp* net);
/* steps (1..GA3C_ACTORS_MAX_STEPS) actor steps: predict on the observations, step every environment, lay the rollouts the
 * step cut out as one batch in environment order and, train != 0 and the batch not empty, train on it (one train step, step
 * += 1).  Returns when they are done.  out_stats (may be NULL) int64[4]: agent steps (n x steps), train calls, rows trained,
 * episodes finished.  The episode ring holds n x GA3C_ACTORS_MAX_STEPS records and is drained into the handle's host
 * queue before the call returns: it cannot overflow. */
int ga3c_dmlp_actors_run(ga3c_dmlp* net, int32_t steps, float learning_rate, float beta, int32_t train, int64_t* out_stats);
/* Takes up to max finished episodes out of the handle's queue, in the order they finished (step, then environment):
 * ProcessAgent.run's (total_reward, total_length), the length counting len(rollout) + 1 per rollout. */
int ga3c_dmlp_actors_episodes(ga3c_dmlp* net, double* total_reward, int64_t* total_length, int32_t max, int32_t* count);
/* For tests: a buffer by name, bytes = its whole size.  Per environment, get and set: "phys" f64[n,4] (x, xdot, th, thdot),
 * "elapsed" i32, "time_count" i32 (0..time_max), "started" i32 (0: no observation yet), "draws" u64 (uniforms drawn so far),
 * "obs" f32[n,4].  Get only, of the last step: "p" f32[n,2], "v" f32[n], "u" f64[n] (-1: no draw), "action" i32, "reward"
 * f64, "done" i32, "cut" i32 (rows of the rollout the step cut, 0: none), "rollout_len" i32 (rows kept for the next one);
 * and its batch: "batch_rows" i32[1], "batch_x" f32[rows,4], "batch_y_r" f32[rows], "batch_a" f32[rows,2].  y_r and a lie
 * in the handle's train staging, which every train-type call on the handle (train, compute_grads, evaluate, upload)
 * overwrites: read the batch before such a call, or what comes back under these two names is that call's rows. */
int ga3c_dmlp_actors_get(ga3c_dmlp* net, const char* name, void* out, int64_t bytes);
int ga3c_dmlp_actors_set(ga3c_dmlp* net, const char* name, const void* in, int64_t bytes);

/* ---- Device actors of the Pendulum network (Config.DEVICE_AGENTS with DEVICE_PENDULUM): n Pendulum-v0 environments
 * on a ga3c_mlp handle.  Signatures, return codes and the step's bookkeeping are those of ga3c_dmlp_actors_* above; what differs
 * is the environment and the action.  What a step restates is ProcessAgent.run_episode / run over EnvironmentPend.Environment:
 * there is no draw for an action -- under CONTINUOUS_INPUT the action is the prediction row p (A = 1 f32), the zero vector on an
 * environment's first ever step -- so "u" stays -1 and "draws" advances only at a reset, which takes two uniforms (th = -pi +
 * 2 pi u0, thdot = -1 + 2 u1; create passes over draws 0..1, draws 2..3 are the first physics).  Torque 2 a, f64 physics
 * (th, thdot), observation [cos th, sin th, thdot] computed in f64 and cast, reward -cost * 0.005 - 1, done after 200 steps.
 * Every episode is 200 steps long, so the environments cut their rollouts on the same steps: one train step of n (time_max + 1)
 * rows every time_max actor steps.
 * create: the network must have S = 3 and A = 1 and n (time_max + 1) <= max_batch (GA3C_EINVAL).  destroy: also done by
 * ga3c_mlp_destroy.  get / set names as above with "phys" f64[n,2], "obs" f32[n,3], "p" f32[n,1], "action" f32[n,1] (the action
 * vector), "batch_x" f32[rows,3], "batch_a" f32[rows,1] (the action vectors). */
int ga3c_mlp_actors_create(ga3c_mlp* net, int32_t n, int32_t time_max, double discount, int64_t seed);
int ga3c_mlp_actors_destroy(ga3c_mlp* net);
int ga3c_mlp_actors_run(ga3c_mlp* net, int32_t steps, float learning_rate, float beta, int32_t train, int64_t* out_stats);
int ga3c_mlp_actors_episodes(ga3c_mlp* net, double* total_reward, int64_t* total_length, int32_t max, int32_t* count);
int ga3c_mlp_actors_get(ga3c_mlp* net, const char* name, void* out, int64_t bytes);
int ga3c_mlp_actors_set(ga3c_mlp* net, const char* name, const void* in, int64_t bytes);

/* ---- DDPG: reference NetworkDDPG.py (USE_DDPG with CONTINUOUS_INPUT), with the replay memory in HBM.
 *   actor   x[B,S] -> actor_fc1 (400) -> actor_norm1 -> relu -> actor_fc2 (300) -> actor_norm2 -> relu -> actor_output (A, tanh)
 *   critic  x -> critic_fc1 (400) -> critic_norm1 -> relu = h;  q = critic_output(relu(h W_fc2 + a W_n2 + b_n2)), W_n2 / b_n2
 *           being the dense layer the reference names critic_norm2; critic_fc2/b is a variable that no kernel reads.
 *   Batch normalisation is gamma (x - moving_mean) / sqrt(moving_variance + 1e-5) + beta; no kernel writes the moving
 *   statistics (0 and 1 after create).
 * A handle of its own with ga3c_mlp's conventions: int return codes, ga3c_last_error(), one HIP stream for every kernel
 * and copy (a prediction sees the weights before or after a step, never a mix; ring writes and train steps are ordered),
 * a lane per prediction in flight, train-type calls serialised.
 *
 * 26 variables, arena order: the actor's ten trainable ones (actor_fc1/W[S,400] /b actor_norm1/beta /gamma actor_fc2/W[400,300]
 * /b actor_norm2/beta /gamma actor_output/W[300,A] /b), the critic's ten (critic_fc1/W[S,400] /b critic_norm1/beta /gamma
 * critic_fc2/W[400,300] /b critic_norm2/W[A,300] /b critic_output/W[300,1] /b), then actor_norm1/moving_mean /moving_variance,
 * actor_norm2/..., critic_norm1/....  `which` of get / set_param: 0 value, 1 target network's value, 2 / 3 optimizer slots
 * (RMSProp ms / mom for the critic, Adam m / v under GA3C_DDPG_CRITIC_ADAM and for the actor), 4 last gradient (get only).
 * Checkpoints: the .npz container of ga3c_net_save: "<var>:0", the target copy under tflearn's second-scope name
 * ("actor_fc1_1/W:0"), the slots as "<var>/RMSProp:0", "/RMSProp_1:0" or "/Adam:0", "/Adam_1:0", and "step", which Adam's
 * bias correction reads.  A file of another network is refused with GA3C_ESTATE and the handle untouched. */
#define GA3C_DDPG_FUTURE_REWARD 1u  /* Config.DDPG_FUTURE_REWARD_CALC: y = r + gamma q' on rows that are not done; else y = r */
#define GA3C_DDPG_LOSS_PAIRED 2u    /* DDPG_CRITIC_LOSS = 'paired': dL/dq_i = (2/B)(q_i - y_i).  Without it the fork's form: y[B]
                                       against q[B,1] broadcasts to [B,B], dL/dq_i = (2/B)(q_i - mean(y)) (NetworkDDPG.py:32,409) */
#define GA3C_DDPG_GRAD_CLIP 4u      /* Config.USE_GRAD_CLIP: tf.clip_by_norm per critic gradient tensor (:354-357) */
#define GA3C_DDPG_CRITIC_ADAM 8u    /* Config.RMSPROP = False: Adam for the critic as for the actor */
#define GA3C_DDPG_OU_NOISE 16u      /* Config.add_OUnoise: the handle's Ornstein-Uhlenbeck process (:463-482) */
#define GA3C_DDPG_NOISE_OWN 0       /* noise_mode: one step of the handle's process (nothing without GA3C_DDPG_OU_NOISE) */
#define GA3C_DDPG_NOISE_GIVEN 1     /*   the caller's noise[A], added to every row */
#define GA3C_DDPG_NOISE_NONE 2      /*   none; the output is wrapped into [-1, 1] elementwise (check_bounds, turnaround) */
typedef struct ga3c_ddpg ga3c_ddpg;
typedef struct ga3c_ddpg_config {
  int32_t device;
  int32_t state_dim;        /* S, 1..64 */
  int32_t num_actions;      /* A, 1..32 */
  int32_t max_batch;        /* rows of one predict / train / replay_add call, 1..4096 */
  int32_t replay_capacity;  /* rows of the ring in HBM, (2 S + A + 2) floats each */
  int32_t predict_lanes;    /* 0 -> 4 */
  uint32_t flags;           /* GA3C_DDPG_* */
  float tau, gamma;         /* Config.tau, Config.gamma */
  float actor_lr, critic_lr;/* Config.actor_lr, Config.critic_lr: factors on the step's learning_rate */
  float rmsprop_decay, rmsprop_momentum, rmsprop_epsilon, grad_clip_norm;
  float ou_sigma, ou_theta, ou_dt;
  int64_t seed;             /* of the handle's normal generator (Config.RANDOM_SEED) */
} ga3c_ddpg_config;

int ga3c_ddpg_create(const ga3c_ddpg_config* cfg, ga3c_ddpg** out);   /* every variable zero, ms 1, moving_variance 1 */
int ga3c_ddpg_destroy(ga3c_ddpg* net);
int32_t ga3c_ddpg_num_params(ga3c_ddpg* net);                          /* 26 */
const char* ga3c_ddpg_param_name(ga3c_ddpg* net, int32_t index);
const char* ga3c_ddpg_target_name(ga3c_ddpg* net, int32_t index);      /* the checkpoint name of the target copy */
int ga3c_ddpg_param_info(ga3c_ddpg* net, const char* name, int64_t* count, int32_t* ndim, int64_t shape[4], int32_t* trainable);
int ga3c_ddpg_get_param(ga3c_ddpg* net, const char* name, int32_t which, float* out, int64_t count);
int ga3c_ddpg_set_param(ga3c_ddpg* net, const char* name, int32_t which, const float* in, int64_t count);
int ga3c_ddpg_get_step(ga3c_ddpg* net, int64_t* step);
int ga3c_ddpg_set_step(ga3c_ddpg* net, int64_t step);
int ga3c_ddpg_save(ga3c_ddpg* net, const char* path);
int ga3c_ddpg_load(ga3c_ddpg* net, const char* path);
/* One step of the handle's OU process: x[A] the new state, n[A] the normal draws it used (each may be NULL). */
int ga3c_ddpg_noise_step(ga3c_ddpg* net, float* x, float* n);
/* x f32[B,S] -> a f32[B,A] = actor(x) + noise, online actor only, one launch. */
int ga3c_ddpg_predict(ga3c_ddpg* net, const float* x, int32_t batch, int32_t noise_mode, const float* noise, float* a);
/* Zero-copy intake, as ga3c_mlp_*: rows of the registered segment by byte offset (4-byte aligned; the first S floats are the
 * state).  The three gather entries have the signatures of the native predictor loops and take GA3C_DDPG_NOISE_OWN; p is the
 * action [B,A], v[B] its first component (predict_p_and_v returns (action, action), NetworkDDPG.py:106-111). */
int ga3c_ddpg_register_host(ga3c_ddpg* net, void* base, int64_t bytes);
int ga3c_ddpg_unregister_host(ga3c_ddpg* net);
int ga3c_ddpg_predict_gather(void* net, const int64_t* offsets, int32_t batch, int32_t u8, float* p, float* v, float* z);
int ga3c_ddpg_predict_gather_begin(void* net, const int64_t* offsets, int32_t batch, int32_t u8, int32_t* ticket);
int ga3c_ddpg_predict_gather_end(void* net, int32_t ticket, int32_t batch, float* p, float* v);
/* The replay ring (replay_buffer.py:16-55): n rows appended, the oldest dropped beyond the capacity.  size: rows held;
 * total: rows ever added (row number t lies in slot t mod capacity).  Both return after the device has read the rows.
 * replay_add_gather reads rows `s[S] | s2[S] | done` (f32) at byte offsets of the registered segment. */
int ga3c_ddpg_replay_add(ga3c_ddpg* net, const float* s, const float* a, const float* r, const float* done, const float* s2,
                         int32_t n, int64_t* size, int64_t* total);
int ga3c_ddpg_replay_add_gather(ga3c_ddpg* net, const int64_t* offsets, const float* r, const float* a, int32_t n, int64_t* size,
                                int64_t* total);
int ga3c_ddpg_replay_get(ga3c_ddpg* net, int64_t slot, float* s, float* a, float* r, float* done, float* s2);
int ga3c_ddpg_replay_size(ga3c_ddpg* net, int64_t* size, int64_t* total);
/* train_DDPG (NetworkDDPG.py:64-98): targets, critic step, action gradient of the updated critic, actor step, soft update of
 * both target networks.  5 launches (6 with GA3C_DDPG_GRAD_CLIP) on the handle's stream and one wait, for q_stats =
 * {max, mean} of q as predicted before the update.  Sums over rows run in row order: the same call on the same state
 * gives the same bits.  train_replay names ring slots; stamp >= 0 is the ring's `total` when they were sampled, and a slot
 * written since is refused with GA3C_ELOST (nothing trained); stamp < 0: no such check. */
int ga3c_ddpg_train(ga3c_ddpg* net, const float* s, const float* a, const float* r, const float* done, const float* s2,
                    int32_t batch, float learning_rate, int32_t noise_mode, const float* noise, float* q_stats);
int ga3c_ddpg_train_replay(ga3c_ddpg* net, const int32_t* slots, int32_t batch, int64_t stamp, float learning_rate,
                           int32_t noise_mode, const float* noise, float* q_stats);
/* For tests: the same kernels stopped after step 3 (the critic's update applied) or step 4 (+ the action gradient and the
 * actor's gradient, not applied); no soft update, the step counter stays. */
int ga3c_ddpg_compute(ga3c_ddpg* net, const float* s, const float* a, const float* r, const float* done, const float* s2,
                      int32_t batch, float learning_rate, int32_t noise_mode, const float* noise, int32_t stop_after,
                      float* q_stats);
/* Rows of the last train-type call: "y", "qt" (q'), "q", "dq" [B]; "c_xh1", "c_c1", "c_dn1", "c_dh1" [B,400]; "c_c2", "c_dt"
 * [B,300]; "a_xh1", "a_a1", "a_dn1", "a_dh1" [B,400]; "a_xh2", "a_a2", "a_dn2", "a_dh2" [B,300]; "a_out", "a_noisy", "g", "do" [B,A]. */
int ga3c_ddpg_fetch(ga3c_ddpg* net, const char* name, float* out, int64_t count);
/* `iters` calls between two events on the handle's stream -> milliseconds: mode 0 predict on ring rows' states, 1 train_replay,
 * both on slots 0 .. batch-1 (the ring must hold them), without noise. */
int ga3c_ddpg_time_resident(ga3c_ddpg* net, int32_t mode, int32_t batch, int32_t iters, float learning_rate, float* elapsed_ms);

/* ---- Proportional prioritised replay on a DDPG handle (Config.PRIORITIZED_REPLAY; tests/per_oracle.py states it
 * addition by addition).  Attached to a created handle by a call of its own, as the device actors are; a handle without
 * priorities runs what it ran before, and every call below returns GA3C_ESTATE on it (as fetch does for "per_w" / "per_td").
 * State: pa[capacity], a slot's priority raised to alpha (0 in a slot never written), max_pa (1 at first, never smaller) and
 * a sample counter.  replay_add* give the slots they write max_pa; rows the ring holds at create get 1.
 * A draw of B rows: the f64 sums of the chunks of 1024 slots, their scan, and per row k the slot at which the running sum
 * first exceeds (k + u(seed, sample number, k)) total / B, u the device actors' counter uniforms with the sample number in the
 * environment's place; a slot may come up more than once.  w_k = (size pa / total)^-beta_is over the batch's largest.
 * A step trains with dL/dq_i = (2/B) w_i (q_i - y_i) and then sets pa[slot_i] = (|y_i - q_i| + eps)^alpha, the last row in
 * batch order where a slot occurs twice, and max_pa = max(max_pa, every new priority).  8 launches (9 with
 * GA3C_DDPG_GRAD_CLIP) on the handle's stream and one wait; no stamp, and nothing can be lost.
 * create: GA3C_EINVAL for alpha outside [0,1], eps <= 0, a NaN, or replay_capacity > 1048576 (1024 chunks); GA3C_ESTATE on a
 * second create and on a handle without GA3C_DDPG_LOSS_PAIRED (under the fork's loss a row has no TD error of its own).
 * destroy: also done by ga3c_ddpg_destroy.  Checkpoints carry no priorities, as they carry no ring. */
int ga3c_ddpg_priorities_create(ga3c_ddpg* net, float alpha, float eps, int64_t seed);
int ga3c_ddpg_priorities_destroy(ga3c_ddpg* net);
/* For tests.  set refuses a negative or NaN entry, a zero in a slot that holds a row, and max_pa <= 0 (GA3C_EINVAL). */
int ga3c_ddpg_priorities_get(ga3c_ddpg* net, float* pa, float* max_pa);
int ga3c_ddpg_priorities_set(ga3c_ddpg* net, const float* pa, float max_pa);
/* One draw: advances the sample counter and does nothing else.  1 <= batch <= max_batch, beta_is >= 0, and the ring holds a
 * row (GA3C_ESTATE otherwise). */
int ga3c_ddpg_sample_prioritized(ga3c_ddpg* net, int32_t batch, float beta_is, int32_t* slots, float* weights);
/* The draw and the step in one call; out_slots (may be null) gets the slots.  GA3C_ESTATE unless the ring holds MORE than
 * `batch` rows (ThreadReplay.sample's rule).  Afterwards fetch knows "per_w" [B] (the last draw's weights, of
 * sample_prioritized too) and "per_td" [B] = |y - q| beside the names above. */
int ga3c_ddpg_train_prioritized(ga3c_ddpg* net, int32_t batch, float beta_is, float learning_rate, int32_t noise_mode,
                                const float* noise, float* q_stats, int32_t* out_slots);
/* `iters` prioritised steps between two events on the handle's stream -> milliseconds, without noise. */
int ga3c_ddpg_time_prioritized(ga3c_ddpg* net, int32_t batch, int32_t iters, float beta_is, float learning_rate,
                               float* elapsed_ms);

/* ---- Twin critics of a DDPG handle (Config.DDPG_TWIN; tests/td3_oracle.py is the same statement in numpy):
 * clipped double-Q with target policy smoothing and a delayed policy update (Fujimoto et al. 2018).  A handle without them runs
 * what it ran before.  With them every train-type call (train, train_replay, train_prioritized, compute, time_resident,
 * time_prioritized, actors_run) runs, with t = step + 1:
 *   a~ = clip(actor_target(s2) + eps, -1, 1), eps[k][i] = (f32) clip(sigma n, -c, c) for row k of the batch and action i, n
 *   Box-Muller in f64 on the device actors' counter uniforms: u1 = 1 - u(seed, t, 2j), u2 = u(seed, t, 2j + 1), j = k A + i,
 *   n = sqrt(-2 ln u1) cos(2 pi u2).  The stream is t: no state, a resumed run draws what the uninterrupted one would.
 *   q' = min(critic_target(s2, a~), critic2_target(s2, a~)), y from it as before.
 *   Both critics step on the same y in the paired form, each with its own optimizer slots and its own clip_by_norm.
 *   Only when t % policy_delay == 0: steps 4-5 against the updated critic 1, the actor's Adam at count t / policy_delay, and
 *   the soft update of all three nets.  On other steps no target and no actor slot changes, and compute's stop_after = 4 does
 *   what 3 does.  The handle's noise process advances once per train-type call either way.
 * 3 launches (4 with GA3C_DDPG_GRAD_CLIP), 5 (6) on a policy step; prioritised steps add their three.
 * The handle then has 38 variables: the 26, then critic2_fc1/W .. critic2_output/b in the critic's order and
 * critic2_norm1/moving_mean, /moving_variance, starting as ga3c_ddpg_create leaves the others; every `which` serves them, and a
 * checkpoint holds their members too.  A twin handle loads only a twin handle's file and a plain handle refuses one
 * (GA3C_ESTATE, handle untouched).  fetch also knows "qt1", "qt2" [B] (the two target critics; "qt" is their min), "t_eps",
 * "t_a" [B,A], "q2", "dq2" [B] and "c2_xh1" .. "c2_dt" as critic 1's "c_*"; GA3C_ESTATE without the twin.  "q", q_stats and
 * "per_td" stay critic 1's.
 * create: GA3C_EINVAL for policy_delay outside [1,16], a negative or NaN target_sigma / target_clip; GA3C_ESTATE on a second
 * create and on a handle without GA3C_DDPG_LOSS_PAIRED (under the fork's loss a row has no target of its own).
 * destroy: also done by ga3c_ddpg_destroy; the handle has its 26 variables again. */
int ga3c_ddpg_twin_create(ga3c_ddpg* net, int32_t policy_delay, float target_sigma, float target_clip, int64_t seed);
int ga3c_ddpg_twin_destroy(ga3c_ddpg* net);

/* ---- Soft actor-critic on a twin handle (Config.DDPG_SOFT; tests/sac_oracle.py is the same statement in numpy):
 * a tanh-Gaussian actor that explores by its own sample, an entropy term in the critics' target and in the actor's loss, and a
 * learned temperature (Haarnoja et al. 2018).  A handle without it runs what it ran before.
 *   Head: actor_output/W is [300, 2A], /b [2A].  With o the raw output, mu = o[:A], ls = clamp(o[A:], ls_min, ls_max),
 *   sigma = exp(ls); no gradient reaches o[A+i] outside the open interval.  Sample: u = fmaf(sigma, eps, mu), a = tanh(u),
 *   logp = sum_i (-eps_i^2 / 2 - ls_i - ln sqrt(2 pi) - ln(1 - a_i^2)) with ln(1 - tanh^2 u) = 2 (ln 2 - |u| - log1p(exp(-2 |u|)))
 *   from u.  eps: 8n's Box-Muller draw, f32, unclipped, j = k A + i for row k and action i.
 * With t = step + 1 every train-type call runs:
 *   a2, logp2 sampled by the ONLINE actor at s2 on stream 2 t of `seed` (the target actor is kept and soft-updated, not read);
 *   q' = min of the two target critics at (s2, a2); v' = q' - alpha logp2, alpha = exp(log_alpha) as it stands;
 *   y = r on a done row or without GA3C_DDPG_FUTURE_REWARD, else fmaf(g, v', r), g the row's discount;
 *   the twin's step of both critics on y.  Only when t % policy_delay == 0: a, logp sampled at s on stream 2 t + 1, both UPDATED
 *   critics at (s, a), per row the smaller one selected (critic 1 on a tie) with g = its dq/da, and the gradient of
 *   J = (1/B) sum_k (alpha logp_k - q_sel,k) -- a MEAN over the rows, where the plain step sums -- through the sample into the
 *   actor; the actor's Adam at count t / policy_delay; then log_alpha's Adam step on -log_alpha (mean_k logp_k + target_entropy),
 *   rows in order, at alpha_lr x learning_rate with the same count; the soft update of all three nets.
 *   The noise arguments of train-type calls are not read, nor are the twin's target_sigma / target_clip.
 * Launches: the twin's, 3 (4 with GA3C_DDPG_GRAD_CLIP), 5 (6) on a policy step, + 3 prioritised; log_alpha's step rides in the
 * actor's weight-gradient launch.
 * Predictions (predict, predict_gather*, actors_run): GA3C_DDPG_NOISE_NONE gives a = tanh(mu), unwrapped; _GIVEN takes the caller's
 * eps[A] for every row; _OWN draws row r's eps[i] as draw c A + i of stream r under seed + 1, c the handle's count of _OWN
 * predictions, which every such call advances by one (a device actor step is one call, its row the environment).  The device
 * actors' last draws are actors_get's "soft_eps" [n][A].  Evaluation episodes act by tanh(mu).
 * The handle then has 39 variables: the twin's 38 with the wider head, then actor_soft/log_alpha (1,), trainable, with Adam's
 * slots.  which = 1 of log_alpha is the value given at create, kept so that every variable has its target copy and checkpoint
 * member; no kernel reads or writes it.  A checkpoint also holds "soft_config", f32 [3]: target_entropy, ls_min, ls_max; a twin
 * file in a soft handle, a soft file in a twin handle, or another soft_config is GA3C_ESTATE with the handle untouched.
 * fetch also knows "s_eps2", "s_a2" [B,A], "s_logp2", "s_vt" [B] (the target) and "s_mu", "s_ls", "s_eps", "s_u" [B,A], "s_logp",
 * "s_q1", "s_q2" [B] (the policy step); GA3C_ESTATE without it.  There "a_noisy" is the sampled action, "g" the selected critic's
 * dq/da, "do" [B,2A] = dJ/dmu | dJ/dls, "qt" min q'; "a_out" is not written.
 * create re-lays the arenas: every other variable keeps its value, target copy, slots and gradient, the head is as
 * ga3c_ddpg_create leaves variables.  GA3C_EINVAL for 2A > 32, a NaN or an infinity, ls_min >= ls_max, alpha_lr < 0;
 * GA3C_ESTATE on a second create, without twin critics, and on a handle that has device actors (so also per-environment noise) or
 * evaluation episodes: the order is twin, soft, then those.  envnoise_create and twin_destroy on a soft handle are GA3C_ESTATE.
 * destroy: the head is [300, A] again, zeroed, and log_alpha is gone (GA3C_ESTATE while device actors or evaluation episodes
 * live); ga3c_ddpg_destroy does it too.
 * info: log_alpha as it stands, target_entropy, the mean logp of the last policy step, the count of _OWN predictions. */
int ga3c_ddpg_soft_create(ga3c_ddpg* net, float log_alpha, float alpha_lr, float target_entropy, float ls_min, float ls_max,
                          int64_t seed);
int ga3c_ddpg_soft_destroy(ga3c_ddpg* net);
int ga3c_ddpg_soft_info(ga3c_ddpg* net, float* log_alpha, float* target_entropy, float* mean_logp, int64_t* predictions);

/* ---- Device actors of a DDPG handle (Config.DEVICE_DDPG; tests/ddpg_actors_oracle.py is the same statement in
 * numpy): n Pendulum-v0 environments in HBM write their transitions into the handle's replay ring and the handle trains on rows
 * it draws from the ring itself, all on its one stream.  Attached to a created handle, as the priorities are.
 * An actor step: the online actor on the n observations plus the step's noise (ga3c_ddpg_predict's kernel); per environment
 * check_bounds(a, 1, -1, turnaround) in f64 on the f32 action, the f64 physics, reward, done and observation, the transition
 * s | a as predicted | (f32) reward | done | s2 into ring slot (rows ever added + i) mod capacity, which gets max_pa under
 * priorities; an episode's record (the f64 sum of its rewards in step order, its transitions + 1) and the reset (two counter
 * uniforms u(seed, environment, draw); the observation is left alone).  The handle's first ever actor step is the host's
 * step(None): the zero action, no prediction, no noise step, no transition.
 * Then, when `train` is set and the ring holds MORE than `batch` rows, `updates` train steps of `batch` rows each: with
 * priorities ga3c_ddpg_train_prioritized's launches; without, slot_k = lo + min(hi - lo - 1, (int64)(u (hi - lo))) with
 * lo = k size / batch, hi = (k + 1) size / batch in int64 and u = u(draw_seed, sample number, k), then ga3c_ddpg_train_replay's
 * launches on those slots.  `batch` starts at max_batch and `draw_seed` at `seed`; both are set by name (below).
 * create: GA3C_EINVAL for n outside [1, min(max_batch, replay_capacity)], updates outside [1,16], or a handle whose
 * state_dim != 3 or num_actions != 1; GA3C_ESTATE on a second create, as is every other call here without actors.
 * destroy: also done by ga3c_ddpg_destroy. */
int ga3c_ddpg_actors_create(ga3c_ddpg* net, int32_t n, int32_t updates, int64_t seed);
int ga3c_ddpg_actors_destroy(ga3c_ddpg* net);
/* steps (1..GA3C_ACTORS_MAX_STEPS) actor steps, everything enqueued with no wait in between and one wait at the end.
 * noise_mode / noise as ga3c_ddpg_predict's, one step of the process per prediction and one per train step's step 4;
 * GA3C_DDPG_NOISE_GIVEN uses the one vector for all of them.  beta_is is read under priorities only.  out_stats[4] (may be
 * null): agent steps, train steps, rows trained, episodes finished; q_stats[2] (may be null): {max q, mean q} of the last
 * train step, untouched when there was none. */
int ga3c_ddpg_actors_run(ga3c_ddpg* net, int32_t steps, float learning_rate, float beta_is, int32_t train, int32_t noise_mode,
                         const float* noise, int64_t* out_stats, float* q_stats);
/* Drains up to `max` finished episodes, oldest first. */
int ga3c_ddpg_actors_episodes(ga3c_ddpg* net, double* total_reward, int64_t* total_length, int32_t max, int32_t* count);
/* By name, `bytes` the buffer's size.  Per environment, get and set: "phys" f64 [n][2], "elapsed" i32, "draws" u64, "obs" f32
 * [n][3]; get only: "action" f32 [n][1] (as predicted), "reward" f64, "done" i32.  Of the handle: "batch" i32 (1..max_batch) and
 * "draw_seed" i64, get and set; "slots" i32 [batch], the last train step's draw, get only. */
int ga3c_ddpg_actors_get(ga3c_ddpg* net, const char* name, void* out, int64_t bytes);
int ga3c_ddpg_actors_set(ga3c_ddpg* net, const char* name, const void* in, int64_t bytes);

/* ---- n-step returns of a DDPG handle's device actors (Config.DDPG_NSTEP; tests/nstep_oracle.py is the same
 * statement in numpy).  Attached to a created handle before its device actors, as the priorities and the twin critics are; a
 * handle without them runs what it ran before.  State: disc[capacity], the discount of the row in each ring slot (gamma at
 * create), and, in the actors' block, every environment's window of its last n transitions.
 * With c = 0, 1, .. the transitions every environment has made since actors_create (step(None) makes none): a step with
 * c < n - 1 writes nothing to the ring and `total` does not move; every later step writes one row per environment as before,
 * for the transition that began at u = c - n + 1: m = the smallest k in 1..n with done_{u+k-1}, n if none;
 * R = sum_{k<m} g_k r_{u+k} in f64 with ascending k, g_0 = 1, g_{k+1} = g_k (f64) gamma; the row is
 * s_u | a_u | (f32) R | done_{u+m-1} | s2_{u+m-1} and disc[slot] = (f32) g_m.  The last n - 1 transitions of an episode so leave
 * with shortened horizons and done = 1, during the first n - 1 steps of the next one; nothing is summed across an episode's
 * end; the last n - 1 transitions before actors_destroy are never written.  At n = 1 the rows are the ones a handle without
 * n-step returns writes and disc stays gamma.  Episode records, reward, done and the train rule are per step and unchanged.
 * A train step whose rows are ring slots (train_replay, train_prioritized, time_*, actors_run) takes y = r + disc[slot] q' on
 * rows that are not done; train and compute, whose rows have no slot, keep the scalar gamma.  replay_add* write disc[slot] =
 * gamma for their rows.  fetch also knows "disc" [B], the discounts the last step's target took (GA3C_ESTATE without n-step);
 * actors_get knows "nstep" i32 (1 without) and "nstep_count" i64, the c of the next step, both get only.
 * create: GA3C_EINVAL for n outside [1, GA3C_DDPG_NSTEP_MAX]; GA3C_ESTATE on a second create, on a handle that has device
 * actors (their windows are sized at actors_create) and on one without GA3C_DDPG_FUTURE_REWARD.
 * destroy: GA3C_ESTATE while the actors live; also done by ga3c_ddpg_destroy.  Checkpoints carry neither disc nor windows, as
 * they carry no ring.
 * get / set: for tests; count must be replay_capacity; set refuses a NaN and a value outside [0,1] (GA3C_EINVAL). */
#define GA3C_DDPG_NSTEP_MAX 16
int ga3c_ddpg_nstep_create(ga3c_ddpg* net, int32_t n);
int ga3c_ddpg_nstep_destroy(ga3c_ddpg* net);
int ga3c_ddpg_nstep_get(ga3c_ddpg* net, float* disc, int64_t count);
int ga3c_ddpg_nstep_set(ga3c_ddpg* net, const float* disc, int64_t count);

/* ---- Distributional critic of a DDPG handle (Config.DDPG_DISTRIBUTIONAL; tests/dist_oracle.py is the same statement
 * in numpy): the critic predicts a categorical distribution over `atoms` fixed returns and is trained by cross-entropy against
 * the projected target distribution (Bellemare et al. 2017); the actor ascends its expectation (Barth-Maron et al. 2018).
 * Attached to a created handle before its initial values are set, as the twin critics are; a handle without it runs what it ran
 * before.  With N = atoms:
 *   support  z_k = fmaf((f32) k, delta, vmin), delta = (vmax - vmin) / (f32)(N - 1), k = 0..N-1: everything in f32, from the f32
 *            vmin and vmax of the call.
 *   head     critic_output/W is [300,N], /b [N]; logits = c2 W + b, p = softmax(logits) with the row maximum subtracted first,
 *            q = sum_k z_k p_k in k order.  q is what "q", q_stats and "per_td" see.
 *   target   p' = softmax of the target critic at (s2, actor_target(s2)); g = 0 on a done row or without GA3C_DDPG_FUTURE_REWARD,
 *            else the row's discount (disc[slot] where a handle with n-step returns trains on ring slots, gamma otherwise);
 *            Tz_j = clip(r + g z_j, vmin, vmax), b_j = (Tz_j - vmin) / delta, m_k = sum_j p'_j max(0, 1 - |b_j - k|) with j
 *            ascending, one thread per (row, k): the C51 projection in gather form, no atomics, continuous in b, and whole where
 *            a b_j is an integer.  "y" = sum_k z_k m_k, "qt" = sum_k z_k p'_k.  Without GA3C_DDPG_FUTURE_REWARD no target net is
 *            evaluated: "d_pt" and "qt" are zero and m_k = max(0, 1 - |b - k|) with b from r alone.
 *   critic   L = (1/B) sum_i w_i ce_i, ce_i = -sum_k m_ik log p_ik, w the importance weights under priorities, else 1;
 *            dz_ik = (w_i / B)(p_ik - m_ik); the delta at the second layer is relu'(t_j) sum_k dz_ik W_o[j][k] in k order, and below
 *            it the backward pass, the weight gradients, the clip and the optimizer are the scalar critic's.
 *   actor    dQ/dlogit_k = p_k (z_k - Q) of the updated critic at (s, actor(s) + noise) stands where the scalar head has its
 *            weight; the rest of steps 4-5 is unchanged.
 *   priorities  pa[slot] = (|y - q| + eps)^alpha on the expectations above.
 * Every train-type call (train, train_replay, train_prioritized, compute, time_resident, time_prioritized, actors_run) runs this
 * step, in the launches of the scalar one: 5 (6 with GA3C_DDPG_GRAD_CLIP, + 3 prioritised).  Priorities, n-step returns and
 * device actors combine with it.  The handle keeps its 26 variables and their names; fetch also knows "d_pt" (p'), "d_m", "d_p",
 * "d_dz" [B,N] and "d_ce" [B] (GA3C_ESTATE without the feature), and "dq" is not written by such a step.
 * Checkpoints: the same members, critic_output/W:0 being [300,N], and "dist_support", f32 [2] = vmin, vmax, beside "step".  A plain
 * file into a distributional handle, a distributional file into a plain handle, another N or another support: GA3C_ESTATE, the
 * handle untouched.
 * create: GA3C_EINVAL for atoms outside [2, GA3C_DDPG_ATOMS_MAX], vmin >= vmax, a NaN or an infinity; GA3C_ESTATE on a second
 * create, on a handle without GA3C_DDPG_LOSS_PAIRED (under the fork's loss a row has no target of its own) and on one with twin
 * critics, as twin_create is on a distributional handle: two distributions have no "min".  The five arenas are re-laid: every
 * variable keeps its value, target copy, slots and gradient, and critic_output/W, /b are as ga3c_ddpg_create leaves variables.
 * destroy: re-lays back to the [300,1] head, zeroed; also done by ga3c_ddpg_destroy.
 * info: atoms = 1 (and a zero support) without the feature; each pointer may be NULL. */
#define GA3C_DDPG_ATOMS_MAX 64
int ga3c_ddpg_dist_create(ga3c_ddpg* net, int32_t atoms, float vmin, float vmax);
int ga3c_ddpg_dist_destroy(ga3c_ddpg* net);
int ga3c_ddpg_dist_info(ga3c_ddpg* net, int32_t* atoms, float* vmin, float* vmax);

/* ---- Evaluation episodes of a DDPG handle (Config.DEVICE_DDPG_EVAL_ENVS; tests/ddpg_eval_oracle.py is the same
 * statement in numpy): n Pendulum-v0 environments that the actor walks without noise from fixed start states, a whole episode
 * in one launch.  Attached to a created handle, as the priorities, the twin critics, the n-step returns and the device actors
 * are; it needs none of them and touches none of them: no actor state, no ring row, no priority, no window, no step of the noise
 * process, no draw counter and not `step`.  A handle without it runs what it ran before.
 * create draws the start states once: environment i starts at th = -pi + 2 pi u(seed, i, 0), thdot = -1 + 2 u(seed, i, 1), u the
 * counter uniform of the device actors, and every run starts there with elapsed = 0, so two evaluations differ by the weights
 * alone.
 * run: `steps` steps of every environment.  A step is the actor (target = 0: the online one, 1: the target copy) on the
 * observation [cos th, sin th, thdot] in f32, ga3c_ddpg_predict's arithmetic with GA3C_DDPG_NOISE_NONE, then the device actors'
 * environment step on that action; total_reward[i] is the f64 sum of environment i's rewards in step order.  One launch on the
 * handle's stream, one copy back, one wait: it reads the weights that exactly one train step left.
 * By name, `bytes` the buffer's size: "start" f64 [n][2], get and set; get only: "phys" f64 [n][2], the physics after the last
 * run; with trace = 1 at create "trace_phys" f64 [n][200][2] (entry t: the physics before step t), "trace_obs" f32 [n][200][3]
 * (what the actor read at step t), "trace_action" f32 [n][200] and "trace_reward" f64 [n][200], whose entries t < the last run's
 * `steps` are that run's (GA3C_ESTATE without the trace); "elapsed_ms" f32, the last run's kernel between two events on the
 * handle's stream, valid until a time_* call records the same events (GA3C_ESTATE before the first run).
 * create: GA3C_EINVAL for n outside [1, GA3C_DDPG_EVAL_MAX_ENVS], a trace that is neither 0 nor 1, or a handle whose state_dim
 * != 3 or num_actions != 1; GA3C_ESTATE on a second create, as is every other call here without evaluation episodes.
 * run: GA3C_EINVAL for steps outside [1, GA3C_DDPG_EVAL_MAX_STEPS] or a target that is neither 0 nor 1.
 * destroy: also done by ga3c_ddpg_destroy. */
#define GA3C_DDPG_EVAL_MAX_ENVS 4096
#define GA3C_DDPG_EVAL_MAX_STEPS 200
int ga3c_ddpg_eval_create(ga3c_ddpg* net, int32_t n, int64_t seed, int32_t trace);
int ga3c_ddpg_eval_destroy(ga3c_ddpg* net);
int ga3c_ddpg_eval_run(ga3c_ddpg* net, int32_t steps, int32_t target, double* total_reward);
int ga3c_ddpg_eval_get(ga3c_ddpg* net, const char* name, void* out, int64_t bytes);
int ga3c_ddpg_eval_set(ga3c_ddpg* net, const char* name, const void* in, int64_t bytes);

/* ---- Per-environment exploration noise of a DDPG handle's device actors (Config.DEVICE_DDPG_NOISE = 'per_env', DESIGN.md 8r;
 * tests/envnoise_oracle.py is the same statement in numpy).  Attached to a handle's device actors; without it every prediction
 * of an actor step adds one step of the handle's shared process to all n rows, as before.
 * State: x[n][A] f32, every environment's Ornstein-Uhlenbeck state, 0 at create; n[n][A], the last normal draws; c, the number
 * of predictions made with it (step(None) predicts nothing and does not count).
 * An actor step under GA3C_DDPG_NOISE_OWN then runs, for environment i and action j, with k = c A + j:
 *   u1 = 1 - u(seed, i, 2k), u2 = u(seed, i, 2k + 1), u the counter uniform of the device actors
 *   n = (f32)(sqrt(-2 ln u1) cos(2 pi u2)) in f64
 *   x_prev = 0 if reset_on_done and environment i's last step was done, else x_i[j]
 *   x' = (f32)(x_prev + theta (0 - x_prev) dt + sigma sqrt(dt) n) in f64 without contraction: ga3c_ddpg_noise_step's expression
 *   action = actor(obs_i)[j] + x' in f32, not wrapped (the environment step wraps)
 * in the predict kernel's epilogue: no further launch, no step of the shared process.  GA3C_DDPG_NOISE_GIVEN and
 * GA3C_DDPG_NOISE_NONE do what they did and leave x, n and c alone.  A train step's step 4 takes one step of the shared process
 * whichever way the predictions are served.  The seed is this state's own: the environments' draws do not move.
 * create: GA3C_EINVAL for reset_on_done outside 0..1; GA3C_ESTATE without device actors, on a second create, and on a handle
 * without GA3C_DDPG_OU_NOISE.  destroy: GA3C_ESTATE without one; also done by ga3c_ddpg_actors_destroy and ga3c_ddpg_destroy.
 * ga3c_ddpg_actors_get / _set by name: "noise_x" f32 [n][A], get and set (finite values, else GA3C_EINVAL); "noise_n" f32
 * [n][A], get only; "noise_count" i64, the c of the next prediction, get and set (>= 0).  GA3C_ESTATE for all three on a handle
 * whose actors have no per-environment noise. */
int ga3c_ddpg_envnoise_create(ga3c_ddpg* net, int64_t seed, int32_t reset_on_done);
int ga3c_ddpg_envnoise_destroy(ga3c_ddpg* net);

/* ---- PopArt on a DDPG handle's critic (Config.DDPG_POPART; tests/popart_oracle.py is the same statement in
 * numpy): adaptive normalisation of the critic's targets that preserves its outputs (van Hasselt et al. 2016).  Attached to a
 * created handle by a call of its own, as the twin critics are; a handle without it runs what it ran before, bit for bit.
 * The handle then has 28 variables: the 26, then critic_popart/mu and critic_popart/nu, f32 (1,), not trainable, 0 and 1 at
 * create: the running first and second moment of the targets.  Every `which` serves them (the slots and the gradient stay zero),
 * the kernels read the value copy and write the same value to the target copy, and a checkpoint holds both copies.
 * sigma = clamp(sqrt(max(nu - mu^2, 0)), sigma_min, sigma_max) in f64 from the stored f32 values.  The critic's output n is a
 * normalised value; the return it stands for is sigma n + mu.  Every train-type call (train, train_replay, train_prioritized,
 * compute, time_resident, time_prioritized, actors_run) then runs, with (mu, nu, sigma) the state before it:
 *   targets  q' = fmaf((f32) sigma, n', mu), n' the target critic's output; y = r on a done row or without
 *            GA3C_DDPG_FUTURE_REWARD, else fmaf(g, q', r) with the row's discount g as before.  "y" and "qt" are in return units.
 *   popart   one workgroup between the target and the critic kernel.  The f64 sums of y and y^2 over the B rows in a fixed
 *            order (thread t of 448 adds rows t, t + 448, .. in that order; the partials fold by the halving tree over 512 leaves);
 *            mu' = (f32)((1 - beta) mu + beta mean(y)), nu' = (f32)((1 - beta) nu + beta mean(y^2)) in f64, stored in both
 *            arenas; sigma' from the STORED mu', nu'; ratio = (f32)(sigma / sigma'), shift = (f32)((mu - mu') / sigma'),
 *            isig' = (f32)(1 / sigma'); critic_output/W <- W ratio and /b <- fmaf(b, ratio, shift) in the value arena and in the
 *            target arena (no slot, no gradient), so that sigma' n + mu' is what sigma n + mu was; "yn" = (y - mu') isig'.
 *   critic   step 3 as before with yn where y was: "q" and "dq" are normalised, the clip and both optimizers are unchanged.
 *   actor    steps 4-5 as before: the actor ascends the normalised value and "g" is dn/da.
 *   soft update as before; both output layers were rescaled alike.
 *   priorities  "per_td" = |yn - n| and pa[slot] = (|yn - n| + eps)^alpha: TD errors free of the returns' scale.
 *   q_stats  in return units: sigma' max(n) + mu' and sigma' mean(n) + mu', mu' and (f32) sigma' coming back in the step's one
 *            copy and one wait.
 * With beta = 0 on fresh statistics every factor is exactly 1 or 0 and the step is the plain paired step's, bit for bit.
 * 6 launches (7 with GA3C_DDPG_GRAD_CLIP, + 3 prioritised).  Priorities, n-step returns, device actors and evaluation episodes
 * combine with it; prediction and evaluation read the actor alone.  fetch also knows "yn" [B] (GA3C_ESTATE without the feature).
 * mu and nu are read and set through ga3c_ddpg_get_param / _set_param by name.  A handle with PopArt loads only such a handle's
 * file and a plain handle refuses one (GA3C_ESTATE, handle untouched).
 * create: GA3C_EINVAL for beta outside [0,1], sigma_min <= 0, sigma_min >= sigma_max, a NaN or an infinity; GA3C_ESTATE on a
 * second create, on a handle without GA3C_DDPG_LOSS_PAIRED (under the fork's loss a row has no target of its own) and on one with
 * twin critics or a distributional critic, as twin_create and dist_create are on a handle with PopArt.
 * destroy: also done by ga3c_ddpg_destroy; the handle has its 26 variables again.
 * info: the value copy's mu and nu and the sigma they give; each pointer may be NULL; GA3C_ESTATE without the feature. */
int ga3c_ddpg_popart_create(ga3c_ddpg* net, float beta, float sigma_min, float sigma_max);
int ga3c_ddpg_popart_destroy(ga3c_ddpg* net);
int ga3c_ddpg_popart_info(ga3c_ddpg* net, float* beta, float* mu, float* nu, float* sigma);

/* ---- The task of a DDPG handle's device actors and evaluation episodes (Config.DEVICE_DDPG_ACTION_BOUND, _TIME_LIMIT,
 * _RESET_OBSERVATION, _REWARD_SCALE, _REWARD_OFFSET; tests/ddpg_task_oracle.py is the same statement in numpy).
 * Without one they step the fork's wrapper, EnvironmentPend.Environment: (WRAP, TERMINAL, 0, 0.005, -1.0), as before and bit for
 * bit.  With one, a non-first actor step of an environment, for the f32 action a as predicted:
 *   bound     v = (f64) a; WRAP: check_bounds(a, 1, -1, turnaround) as before; CLIP: v < -1 -> -1, v > 1 -> 1.  Then the
 *             physics and the cost on u = 2 v, unchanged.
 *   reward    -cost * reward_scale + reward_offset in f64, in that order; at (0.005, -1.0) the same bits as before.
 *   the end   ended = elapsed' >= 200; terminal = ended under TERMINAL, never under TRUNCATE.
 *   the row   obs | a as predicted | (f32) reward | terminal ? 1 : 0 | obs', obs' the observation after the step and before
 *             any reset: under TRUNCATE the state the bootstrap reads.
 *   after it  the actor field "done", the episode record, the reset and its draws, and reset_on_done of the per-environment
 *             noise follow `ended`.  With reset_observation the field "obs" then becomes the observation of the reset physics
 *             and the next row starts there; without it the observation stays, as before.
 *   n-step    the sum is cut at `ended`; the row's done is the terminal of the last transition summed: a row cut by a
 *             truncating time limit is s_u | a_u | R | 0 | s2_{u+m-1} with disc = (f32) gamma^m.
 *   evaluation episodes: only the reward differs.
 * The train step reads r, done, s2 and the discount from the ring as before and does not know of the task; the support of a
 * distributional critic is the caller's to fit to the reward.  No further launch per actor step, no flag, no field.
 * create: GA3C_EINVAL for a bound or time_limit outside 0..1, reset_observation outside 0..1, a reward_scale that is not finite
 * or not > 0, a reward_offset that is not finite; GA3C_ESTATE on a second create and on a handle that has device actors or
 * evaluation episodes, which choose their kernels when they are made.
 * destroy: GA3C_ESTATE without a task or with live actors or evaluation episodes; ga3c_ddpg_destroy drops the task.
 * info: each pointer may be NULL; GA3C_ESTATE without a task. */
#define GA3C_DDPG_TASK_WRAP 0      /* bound */
#define GA3C_DDPG_TASK_CLIP 1
#define GA3C_DDPG_TASK_TERMINAL 0  /* time_limit */
#define GA3C_DDPG_TASK_TRUNCATE 1
int ga3c_ddpg_task_create(ga3c_ddpg* net, int32_t bound, int32_t time_limit, int32_t reset_observation, double reward_scale,
                          double reward_offset);
int ga3c_ddpg_task_destroy(ga3c_ddpg* net);
int ga3c_ddpg_task_info(ga3c_ddpg* net, int32_t* bound, int32_t* time_limit, int32_t* reset_observation, double* reward_scale,
                        double* reward_offset);

#ifdef __cplusplus
}
#endif
#endif /* GA3C_ABI_H */
