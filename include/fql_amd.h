/*
 * fql_amd.h -- C ABI of the MI355X-native FQL step engine (libfql_amd.so).
 *
 * This is the drop-in boundary for ONE path of zhouzypaul/fql: the FQL gradient step
 * (FQLAgent.update / total_loss / sample_actions / compute_flow_actions, agents/fql.py:94-171)
 * plus the batch source feeding it (utils/datasets.py:64-100).  Every entry point cites the
 * reference interface it replaces (paths relative to the reference repo).  The reference is pure
 * Python, so "what the reference's FFI would bind" is a ctypes stub: see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success, a negative FQL_E_* code on failure; the message is
 *     available from fql_last_error(handle) (or fql_last_error(NULL) for create failures).
 *     The Python mirror turns FQL_E_INVALID into ValueError and everything else into
 *     RuntimeError (the reference surfaces shape errors as Python exceptions at jit-trace time).
 *   - all tensors are fp32, contiguous, row-major.  Batch / observation / action / noise
 *     pointers may be DEVICE pointers (e.g. torch-ROCm tensor.data_ptr()) or HOST pointers;
 *     the engine detects which (hipPointerGetAttributes) and stages host memory itself.
 *     Pointers are borrowed for the duration of the call only (device pointers: until the work
 *     enqueued by the call has run on `stream`).
 *   - `stream` is a hipStream_t passed as void*.  NULL = the engine's own (non-blocking) stream: nothing
 *     orders it against work the caller has in flight elsewhere, so device pointers passed with a NULL
 *     stream must already be complete, and calls that write a DEVICE output on the NULL stream finish it
 *     before returning.  FQL_STREAM_LEGACY ((void*)1, the value of hipStreamLegacy) = the legacy default
 *     stream - what torch's *default* stream is (its handle reads 0 and cannot be told from NULL): pass it
 *     when the batch was produced on that stream.  Calls on one handle must be serialised by the caller;
 *     the engine never synchronises the host except where documented (host output pointers, get_* calls).
 *   - the engine owns params, Adam state, the target network and all workspaces in HBM.
 *     There is NO CPU fallback: without a HIP device fql_create fails with FQL_E_NODEVICE.
 */
#ifndef FQL_AMD_H
#define FQL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FQL_ABI_VERSION 1

#define FQL_OK 0
#define FQL_E_INVALID (-1)  /* bad argument / shape mismatch against the config captured at create */
#define FQL_E_NODEVICE (-2) /* no HIP device / wrong architecture */
#define FQL_E_HIP (-3)      /* a HIP runtime call failed */
#define FQL_E_STATE (-4)    /* call order violated (e.g. update_end without update_begin) */
#define FQL_E_NOTFOUND (-5) /* unknown leaf name */

#define FQL_STREAM_LEGACY ((void*)1) /* == hipStreamLegacy: the legacy default (NULL) stream, e.g. torch's default stream */

#define FQL_MAX_HIDDEN 8
#define FQL_NUM_INFO 13

typedef struct fql_engine* fql_handle;
typedef struct fql_group_s* fql_group;

/* agents/fql.py:249-270 get_config() -- same keys, same defaults (see fql_default_config). */
typedef struct fql_config {
    int32_t obs_dim;                         /* config['ob_dims'][0]; state-based path only        */
    int32_t act_dim;                         /* config['action_dim']                               */
    int32_t num_actor_hidden;                /* len(actor_hidden_dims), <= FQL_MAX_HIDDEN          */
    int32_t actor_hidden[FQL_MAX_HIDDEN];    /* actor_hidden_dims  (512,512,512,512)               */
    int32_t num_value_hidden;                /* len(value_hidden_dims)                             */
    int32_t value_hidden[FQL_MAX_HIDDEN];    /* value_hidden_dims  (512,512,512,512)               */
    int32_t layer_norm;                      /* critic LayerNorm (True)                            */
    int32_t actor_layer_norm;                /* actor LayerNorm (False)                            */
    float lr;                                /* 3e-4                                               */
    float discount;                          /* 0.99                                               */
    float tau;                               /* 0.005                                              */
    float alpha;                             /* 300.0                                              */
    int32_t q_agg;                           /* 0 = 'mean', 1 = 'min'                              */
    int32_t flow_steps;                      /* 10                                                 */
    int32_t normalize_q_loss;                /* False                                              */
    int32_t batch_size;                      /* 256: rows per update on this device (multiple of 16) */
    int32_t precision;                       /* 0 = fp32 MFMA (exact fp32 fma chains; default).  2 = "bf16x3": every fp32 operand of the dense
                                                contractions is split into hi + lo bf16 and a b = a_hi b_hi + a_hi b_lo + a_lo b_hi runs on the
                                                bf16 matrix cores with fp32 accumulation (~2^-17 relative per product; parameters, activations,
                                                gradients and the optimizer stay fp32).  1 (plain bf16) is rejected: it cannot hold the 1e-4 loss bound */
    int32_t encoder;                         /* 0 = state observations; 1 = impala_small, 2 = impala (utils/encoders.py:104,106; stacks 16/32/32, 1 or 2 blocks): obs_dim is
                                                ignored, observations are uint8 [B, img_h, img_w, img_c] (agents/fql.py:196-202) */
    int32_t img_h, img_w, img_c;             /* image shape after frame stacking (e.g. 64, 64, 9); img_h, img_w multiples of 8 */
    int32_t reserved[3];
} fql_config;

/* The five random tensors one update draws (agents/fql.py:24,49-54,62-63,82,143-150; derivation in
 * SURVEY.md section 8a).  Any pointer may be NULL: that tensor then comes from the engine's own
 * counter-based RNG (Philox4x32-10 keyed by the create seed and the step counter). */
typedef struct fql_noise {
    const float* eps1; /* [B, act]  critic_loss: sample_actions(next_observations) noise */
    const float* x0;   /* [B, act]  actor_loss: x_0                                      */
    const float* t;    /* [B]       actor_loss: t ~ U[0,1)                               */
    const float* z;    /* [B, act]  actor_loss: distillation noises                      */
    const float* eps2; /* [B, act]  actor_loss: sample_actions(observations) noise (mse)  */
} fql_noise;

/* info13 order == the reference's info dict (agents/fql.py:39-44,85-92,103-108;
 * utils/flax_utils.py:151-157):
 *  0 critic/critic_loss 1 critic/q_mean 2 critic/q_max 3 critic/q_min 4 actor/actor_loss
 *  5 actor/bc_flow_loss 6 actor/distill_loss 7 actor/q_loss 8 actor/q 9 actor/mse
 *  10 grad/max 11 grad/min 12 grad/norm */
const char* fql_info_name(int i);

int fql_abi_version(void);
void fql_default_config(fql_config* cfg);
const char* fql_last_error(fql_handle h);

/* FQLAgent.create(seed, ex_observations, ex_actions, config)  agents/fql.py:173-246.
 * Builds the 4 networks (critic x2 members, target critic x2, actor_bc_flow, actor_onestep_flow),
 * Glorot-uniform kernels / zero biases / LN scale 1 bias 0 (utils/networks.py:9-11), target := critic
 * (agents/fql.py:241-242), Adam state zero, step = 1 (utils/flax_utils.py:81). */
int fql_create(const fql_config* cfg, uint64_t seed, fql_handle* out);
int fql_destroy(fql_handle h);
/* Re-size the per-step workspace for another batch size (params/optimizer state are kept). */
int fql_set_batch_size(fql_handle h, int batch_size);

/* Parameter / optimizer-state access by the reference's leaf path (utils/flax_utils.py:16-50 ModuleDict
 * naming), e.g. "modules_critic/value_net/Dense_0/kernel" (shape [2,in,out]),
 * "modules_actor_bc_flow/mlp/Dense_4/bias".  Host pointers, reference shapes, synchronous. */
int fql_num_leaves(fql_handle h);
int fql_leaf_info(fql_handle h, int index, char* name, int name_cap, int* ndim, int64_t shape[4]);
int fql_get_param(fql_handle h, const char* leaf, float* host_out, size_t n);
int fql_set_param(fql_handle h, const char* leaf, const float* host_in, size_t n);
/* which: 0 = Adam mu, 1 = Adam nu (optax ScaleByAdamState; utils/flax_utils.py:120-130) */
int fql_get_opt_state(fql_handle h, int which, const char* leaf, float* host_out, size_t n);
int fql_set_opt_state(fql_handle h, int which, const char* leaf, const float* host_in, size_t n);
/* optax count (0 at create) and TrainState.step (1 at create, utils/flax_utils.py:81).  fql_set_step also positions the device RNG at
 * the adam_count-th update (the RNG's step counter advances with adam_count), so an agent restored from a checkpoint continues the
 * saved agent's draws (the reference keeps its rng key in the checkpoint). */
int fql_get_step(fql_handle h, int64_t* adam_count, int64_t* train_step);
int fql_set_step(fql_handle h, int64_t adam_count, int64_t train_step);

/* FQLAgent.update(batch)  agents/fql.py:122-133 (+ utils/flax_utils.py:120-159 grad stats, Adam;
 * agents/fql.py:113-120 Polyak from the PRE-step critic).  batch keys observations/actions/rewards/
 * masks/next_observations of utils/datasets.py:68-100 ('terminals' is unused by FQL).
 * `info13` may be NULL (async, read later with fql_read_info); a HOST info13 pointer makes the call
 * synchronous. */
int fql_update(fql_handle h, const float* observations, const float* actions, const float* rewards,
               const float* masks, const float* next_observations, int batch_size,
               const fql_noise* noise, float* info13, void* stream);
/* The two halves of fql_update for data-parallel runs: begin = forward + backward (gradients of the
 * LOCAL batch mean land in the buffer fql_grad_buffer returns), the caller all-reduces that buffer
 * (RCCL via torch.distributed), end = grad stats + Adam + Polyak.  fql_set_grad_scale(1/world) turns
 * the all-reduced SUM into the mean inside the optimizer kernel. */
int fql_update_begin(fql_handle h, const float* observations, const float* actions, const float* rewards,
                     const float* masks, const float* next_observations, int batch_size,
                     const fql_noise* noise, void* stream);
int fql_update_end(fql_handle h, float* info13, void* stream);
/* Overlapped variant of fql_update_begin for data-parallel runs: the same update enqueued as single-lane graphs on TWO
 * streams.  When the call returns, everything gradient bucket 0 (fql_grad_buckets: both critic members + the BC flow
 * actor) depends on is on `stream1`, everything bucket 1 (the one-step actor) depends on is on `stream0`: all-reduce
 * bucket 0 on stream1 while stream0 still runs the Euler chain, bucket 1 on stream0, make stream0 wait for stream1,
 * then fql_update_end(stream0).  Returns FQL_E_STATE if the engine has no two-lane program (then use fql_update_begin). */
int fql_update_begin_split(fql_handle h, const float* observations, const float* actions, const float* rewards,
                           const float* masks, const float* next_observations, int batch_size,
                           const fql_noise* noise, void* stream0, void* stream1);
int fql_update_from_dataset_begin_split(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi,
                                        const fql_noise* noise, void* stream0, void* stream1);
/* The optimizer half on the two streams of the split begin: Adam (+ Polyak) of the critic and the BC flow - gradient bucket 0 - and the
 * refresh of the Euler chain's weight copies on stream1 (behind bucket 0's all-reduce, which the caller enqueued there), Adam of the
 * one-step actor - bucket 1 - and the step bookkeeping on stream0 (behind bucket 1's all-reduce); stream0 ends behind both.  Same
 * result as fql_update_end. */
int fql_update_end_split(fql_handle h, float* info13, void* stream0, void* stream1);
/* offsets / lengths (in floats) of the two gradient buckets inside the buffer fql_grad_buffer returns */
int fql_grad_buckets(fql_handle h, size_t offsets[2], size_t lengths[2]);
int fql_grad_buffer(fql_handle h, void** device_ptr, size_t* num_floats);
int fql_set_grad_scale(fql_handle h, float scale);
/* Data-parallel replicas are created with the SAME seed (identical initial parameters); stream_id (the rank) is mixed into the
 * key of the device RNG so that every rank draws different indices inside its shard and different noise (agents/fql.py:24,49-54,
 * 62-63 draw per-sample noise: ranks must not repeat each other's).  0 = the single-process stream. */
int fql_set_rng_stream(fql_handle h, uint64_t stream_id);

/* FQLAgent.total_loss(batch, grad_params=None)  agents/fql.py:94-111 -- the validation probe of
 * main.py:284: pure forward, no state change.  loss = critic_loss + actor_loss; info10 = the first 10
 * info entries.  Synchronous. */
int fql_total_loss(fql_handle h, const float* observations, const float* actions, const float* rewards,
                   const float* masks, const float* next_observations, int batch_size,
                   const fql_noise* noise, float* loss, float* info10, void* stream);

/* FQLAgent.sample_actions(observations, seed)  agents/fql.py:135-153: clip(onestep(obs, noise)).
 * `noise` [n, act] or NULL (engine RNG keyed by `seed`); `out` [n, act] device or host. */
int fql_sample_actions(fql_handle h, const float* observations, int n, const float* noise, uint64_t seed,
                       float* out, void* stream);
/* FQLAgent.compute_flow_actions(observations, noises)  agents/fql.py:155-171 (Euler, then clip). */
int fql_flow_actions(fql_handle h, const float* observations, const float* noises, int n, float* out,
                     void* stream);
/* agent.network.select(module)(...)  utils/flax_utils.py ModuleDict / TrainState.select: forward of ONE module, stored parameters,
 * caller rows.  No state change.  `module` is the reference's module name without "modules_":
 *   "critic", "target_critic" (FQL, IFQL, ReBRAC, SAC, IQL, IQL-diffusion; utils/networks.py Value.__call__(observations, actions)):
 *     observations [n, obs], actions [n, act], times NULL; out [2, n], the ensemble member first as in the reference;
 *   "value" (IFQL, IQL, IQL-diffusion; Value.__call__(observations)): observations [n, obs], actions and times NULL; out [n];
 *   "actor_bc_flow" (FQL), "actor_flow" (IFQL) (ActorVectorField.__call__(observations, actions, times)): the input row is
 *     [obs | actions | times], times [n], any real t; out [n, act], NOT clipped (the clip is sample_actions' / compute_flow_actions');
 *   "actor_onestep_flow" (FQL; ActorVectorField.__call__(observations, noises)): actions [n, act], times NULL; out [n, act], not clipped.
 * n >= 1, any value: the rows run in chunks of <= 4096 on 16-row tiles, and row j of a call is bit for bit the single-row call on row j.
 * Pointers are device or host; `stream` as elsewhere (NULL: the engine's own stream, a device `out` is finished before return).  Like
 * every entry point the call first waits for the handle's updates on the engine's own queues and for its group's last update, so it
 * sees the latest parameters.  A bf16x3 FQL handle runs the split forward its samplers run.  The query's buffers and programs are its
 * own: no update, loss-probe or sampling workspace changes.
 * FQL_E_NOTFOUND: a module the handle's kind does not have (fql_last_error lists the kind's modules).  FQL_E_INVALID: a NULL pointer the
 * module needs, a non-NULL pointer it does not take, n <= 0.  FQL_E_STATE: BC and CFGRL handles, visual handles.
 * Out of scope and refused: the Gaussian "actor" / "target_actor" of ReBRAC, SAC and IQL (the reference returns a distribution object;
 * sample_actions with temperature 0 gives the clipped mode); IQL-diffusion's "actor", BC's policy and CFGRL's "actor_flow" (their inputs
 * carry host-built embeddings and the unc_embed row); visual agents (the reference runs the module's encoder first); a params= override. */
int fql_module_forward(fql_handle h, const char* module, const float* observations, const float* actions,
                       const float* times, int n, float* out, void* stream);

/* Dataset.create / ReplayBuffer (utils/datasets.py:36-62,435-495): the transition arrays live in HBM.
 * `capacity` >= n rows are allocated (main.py:112-114 uses max(2M, n+1) for online runs). */
int fql_dataset_upload(fql_handle h, int64_t n, int64_t capacity, const float* observations,
                       const float* actions, const float* rewards, const float* masks,
                       const float* next_observations);
/* ReplayBuffer.add_transition (utils/datasets.py:483-491): ring insert of one row; returns new size via
 * fql_dataset_size. */
int fql_dataset_add(fql_handle h, const float* observation, const float* action, float reward, float mask,
                    const float* next_observation);
int fql_dataset_size(fql_handle h, int64_t* size, int64_t* pointer);
/* Dataset.sample(batch_size, idxs) + update (main.py:201,216) without leaving the device:
 * idx [B] int64 (device or host) or NULL = uniform indices from the engine RNG
 * (utils/datasets.py:64-66).  [lo, hi) restricts sampling to a shard of the rows (data-parallel:
 * rank r owns [r*n/W, (r+1)*n/W)); pass 0, 0 for the whole dataset. */
int fql_update_from_dataset(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi,
                            const fql_noise* noise, float* info13, void* stream);
int fql_update_from_dataset_begin(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi,
                                  const fql_noise* noise, void* stream);

/* Visual datasets (encoder != 0; utils/datasets.py:73-112): the uint8 frames [n, img_h, img_w, img_c / frame_stack] live in HBM;
 * a batch row is built on the device as Dataset.sample does: `frame_stack` frames ending at the sampled index, clamped to the first
 * index of its episode (initial_locs from `terminals`, utils/datasets.py:58-62), concatenated on the channel axis; next_observations
 * shifts by one and ends with next_frames[idx]; with probability p_aug per BATCH both are edge-padded by 3 and cropped at a
 * per-sample offset in [0, 6]^2 (Dataset.augment).  Device or host pointers. */
int fql_dataset_upload_frames(fql_handle h, int64_t n, const uint8_t* frames, const uint8_t* next_frames,
                              const float* actions, const float* rewards, const float* masks,
                              const float* terminals, int frame_stack, float p_aug);
/* fql_update_from_dataset for frames.  crop_froms: int32 [B, 2] (y, x) offsets as Dataset.augment draws them (3, 3 = identity),
 * or NULL = the engine's RNG (coin with p_aug, then offsets).  fql_update_from_dataset on a frames dataset == this with NULL. */
int fql_update_from_frames(fql_handle h, const int64_t* idx, const int32_t* crop_froms, int batch_size, int64_t lo,
                           int64_t hi, const fql_noise* noise, float* info13, void* stream);

/* JAX-compatible noise generated on the device (agents/fql.py:24,49-54,62-63,82,125,143-150): keys10 = the five uint32[2] keys the
 * reference's split chain derives for (eps1, x0, t, z, eps2) of one update (the chain itself is a dozen 2-word hashes: host side,
 * fql_amd/jax_prng.py fql_update_keys); partitionable = the jax_threefry_partitionable layout (0: original counter layout).
 * The tensors are written on `stream` into engine-owned device buffers and *out is filled with pointers to them: pass it as the
 * `noise` argument of the next update call on the same stream (valid until the next call of this function or the next update
 * given host noise).  No host tensor crosses PCIe. */
int fql_noise_from_jax_keys(fql_handle h, const uint32_t* keys10, int partitionable, int batch_size, fql_noise* out, void* stream);

/* ---- online fine-tuning hooks (main.py:217-272) ------------------------------------------------------------------------------
 * ReplayBuffer.create_from_initial_dataset(dataset, size) (utils/datasets.py:457-473, main.py:111-115): grow the uploaded dataset
 * (state or frames) to a ring of `capacity` >= current rows, new rows zero; size and pointer stay at the row count.  For frames
 * the episode starts are NOT recomputed on insert, as in the reference (Dataset.__init__ computes initial_locs once): rows
 * inserted later clamp their frame stack at the last episode start of the initial data. */
int fql_dataset_reserve(fql_handle h, int64_t capacity);
/* ReplayBuffer.add_transition (utils/datasets.py:483-491) for a frames dataset: one uint8 frame pair [img_h, img_w, img_c / frame_stack]
 * + action, reward, mask into the ring.  Device or host pointers. */
int fql_dataset_add_frames(fql_handle h, const uint8_t* frame, const uint8_t* next_frame, const float* action, float reward,
                           float mask);
/* ReplayBuffer.create(example_transition, size) (utils/datasets.py:441-455; main.py:106-109, --balanced_sampling): a second,
 * initially empty ring of `capacity` rows in HBM beside the training dataset; state rows or uint8 frames as the agent has them
 * (frames: after fql_dataset_upload_frames, whose frame_stack and p_aug it shares, main.py:117-120). */
int fql_replay_create(fql_handle h, int64_t capacity);
int fql_replay_add(fql_handle h, const float* observation, const float* action, float reward, float mask,
                   const float* next_observation);
int fql_replay_add_frames(fql_handle h, const uint8_t* frame, const uint8_t* next_frame, const float* action, float reward,
                          float mask);
int fql_replay_size(fql_handle h, int64_t* size, int64_t* pointer);
/* main.py:255-259 + :216: batch = concat(train_dataset.sample(B // 2), replay_buffer.sample(B // 2)); agent.update(batch), without
 * leaving the device.  idx_dataset / idx_replay: int64 [B / 2] each (device or host), or both NULL = uniform draws over the
 * dataset rows / the replay ring's `size` rows from the engine RNG.  crop_froms (frames only): int32 [B, 2] or NULL = one
 * augmentation coin per HALF (two sample() calls in the reference), offsets per row.  batch_size must be even and equal to the
 * workspace batch; FQL_E_INVALID while the replay ring is empty. */
int fql_update_balanced(fql_handle h, const int64_t* idx_dataset, const int64_t* idx_replay, const int32_t* crop_froms,
                        int batch_size, const fql_noise* noise, float* info13, void* stream);

/* Blocking read of the info of the last update (the reference reads lazily at log time, main.py:276). */
int fql_read_info(fql_handle h, float* info13_host);
/* Host wait for everything the engine has enqueued: its HIP stream AND the hardware queues of its own that updates with stream = NULL
 * run on (a hipStreamSynchronize / hipDeviceSynchronize of the caller does not see those queues; every other entry point of this header
 * waits for them by itself before it touches the engine's buffers).  `mode` (out, may be NULL): 1 if the last fql_update* call went to
 * the engine's own queues, 0 if it ran as a captured graph on a stream.  (jax.block_until_ready on the agent, main.py:216.) */
int fql_synchronize(fql_handle h, int* mode);
/* Lazy infos, as the reference's `agent, info = agent.update(batch)` returns them (device scalars nobody waits for until they are
 * logged, main.py:216,276): fql_info_enqueue, called right after an update on the same stream, snapshots that update's 13 scalars
 * asynchronously (no host synchronisation) and returns a ticket; fql_info_wait blocks until the snapshot has landed and copies it
 * out.  A ticket expires (FQL_E_STATE) once 64 later tickets have been taken. */
int fql_info_enqueue(fql_handle h, void* stream, uint64_t* ticket);
int fql_info_wait(fql_handle h, uint64_t ticket, float* info13_host);

/* ---- agent groups: K agents of one structure trained side by side (seed / alpha sweeps, README "Tips for hyperparameter tuning") ----
 * A group advances its members with ONE fused update program: every launch of a member's update carries the tasks of all K members
 * (concatenated task tables, or blockIdx.y = member), captured as one graph with a single agent's lanes.  Each task keeps its arguments
 * and tile shapes, so a member's trajectory is bitwise the one it has alone (same seed, alpha, rows and noise).  Members stay ordinary
 * handles: every entry point above works on them.  Errors of the fql_group_* calls are reported by fql_last_error(NULL).
 *
 * fql_group_create: `members` [k], k >= 1, distinct, in no other group.  Members are state agents (encoder 0) with precision 0, the same
 * config except alpha (and the create seed), the same batch size, and structurally identical update programs (launch count, kernels,
 * grids, lanes, waits).  Anything else: FQL_E_INVALID.
 * Out of scope and refused: visual or bf16x3 members, members that differ in anything but seed and alpha.  Data-parallel halves and
 * the engine's own queues (stream = NULL updates of a single agent) are not group paths.  Balanced sampling is a group path for SAC
 * groups alone (fql_sac_group_update_balanced, below): a member's replay ring stays the member's own, filled through the member's
 * fql_replay_add; no group call inserts into a ring.
 * While a handle belongs to a group, fql_set_batch_size and fql_destroy on it return FQL_E_STATE. */
int fql_group_create(const fql_handle* members, int k, fql_group* out);
/* Waits for the group's last update and releases the members (they are plain handles again; nothing is freed of them). */
int fql_group_destroy(fql_group g);
/* fql_update_from_dataset of every member in one fused update: member i samples its rows from ITS OWN uploaded dataset, idx + i * B
 * ([k][B] int64, device or host) or NULL = each member's device RNG; the noise always comes from each member's device RNG.
 * info13xk: [k][13] (device or host; host = synchronous) or NULL.  `stream` as elsewhere: NULL = the group's own stream.
 * Ordering: (0) the update is ordered after the group's previous call (update or sampling), also where that one ran on another stream.
 * (1) the update is ordered after all work submitted earlier through any member: a member's queued engine-queue updates are
 * drained and the group's stream waits for the member's stream (work the caller enqueued on streams of its own is the caller's to order).
 * (2) every member entry point called afterwards sees this update's results without an explicit synchronise (fql_get_param /
 * fql_set_param included): it waits for the group's update first (fql_info_enqueue: a stream dependency, no host wait). */
int fql_group_update_from_dataset(fql_group g, const int64_t* idx, int batch_size, float* info13xk, void* stream);
/* Host wait for the group's last update or sampling call. */
int fql_group_synchronize(fql_group g);
/* fql_sample_actions of every member in one fused call: member i acts on ITS OWN rows, observations + i * n * obs_dim ([k][n][obs_dim]),
 * with the noise noises + i * n * act_dim ([k][n][act_dim]) or, noises NULL, its device draw keyed by seeds[i] ([k], host; may be NULL
 * only with noises); out [k][n][act_dim].  Pointers are device or host each (host out = synchronous; device out on a caller's stream =
 * asynchronous; `stream` NULL = the group's own stream, finished before the call returns).  Every launch of a member's call carries
 * all k members' rows (the assemble and extract launches with blockIdx.y = member, the layers over concatenated task tables), issued as
 * direct launches: the launch count of a call does not depend on k.  Rows are chunked and seeded draws keyed exactly as the member's
 * own call does it (<= 4096 rows per member and chunk, seeds[i] + first row of the chunk), so out[i] is bitwise what
 * fql_sample_actions(member i, ..., seeds[i], ...) returns.  No state of a member changes.
 * Ordering: as fql_group_update_from_dataset - after the group's last call, after everything submitted earlier through a member, and
 * every member entry point called afterwards waits for this call.
 * FQL_E_INVALID: NULL group, n <= 0, NULL observations or out, NULL seeds without noises. */
int fql_group_sample_actions(fql_group g, const float* observations, int n, const float* noises, const uint64_t* seeds, float* out,
                             void* stream);
/* fql_flow_actions of every member likewise (the Euler flow of each member's BC actor on the caller's noises, which are required). */
int fql_group_flow_actions(fql_group g, const float* observations, const float* noises, int n, float* out, void* stream);
/* Kernel launches of one fused sampling call (flow != 0: of one flow call) on a single chunk, counted from the built program. */
int fql_group_sample_stats(fql_group g, int flow, int64_t* launches_per_call);

/* Introspection for tests / bench: per-update kernel-launch count, algorithmic MAC count per update
 * (SURVEY.md section 8d figure), and the engine's HIP stream. */
int fql_stats(fql_handle h, int64_t* launches_per_update, int64_t* macs_per_update, int64_t* param_count);
void* fql_stream(fql_handle h);

/* ---- IFQL: implicit flow Q-learning (agents/ifql.py), the flow variant of IDQL, on the same engine ----
 * State observations and fp32 only.  Networks (agents/ifql.py:188-225): "modules_value/value_net/..." (a 1-member Value: leaves are
 * UNSTACKED [in, out]), "modules_critic/value_net/..." and "modules_target_critic/value_net/..." (stacked [2, ...] as in FQL),
 * "modules_actor_flow/mlp/..." (FQL's BC flow network).  Glorot-uniform kernels, zero biases, target := critic.
 * An IFQL handle is an ordinary fql_handle: destroy, set_batch_size, leaf / param / opt-state / step access, fql_update,
 * fql_update_from_dataset (device-drawn and explicit rows), dataset upload / add / reserve / size, fql_total_loss (writes 9 infos:
 * loss = value + critic + actor), fql_sample_actions, fql_flow_actions, info enqueue / wait, fql_read_info, fql_synchronize, fql_stats
 * and fql_stream work on it.  Differences:
 *   - info buffers stay 13 floats: slots 0-11 hold the 12 IFQL infos (fql_handle_info_name), slot 12 is 0;
 *   - fql_noise: only x0 [B, act] and t [B] are read; any other non-NULL pointer is FQL_E_INVALID;
 *   - fql_sample_actions: per observation, num_samples noises through the Euler flow of actor_flow, clipped to [-1, 1], scored by
 *     min(q1, q2) of the critic, the first argmax kept (agents/ifql.py:123-155).  noise is [n, num_samples, act] or NULL (engine RNG).
 *     n > 1 is an extension (the reference takes one observation): row by row equal to n single calls with the same noises;
 *   - alpha, q_agg and normalize_q_loss of fql_config are ignored.
 * Refused: encoder != 0 or precision != 0 at create (FQL_E_INVALID); on an IFQL handle fql_update_begin* / _end*, fql_grad_buckets, frame
 * uploads / updates, fql_noise_from_jax_keys, the replay ring and balanced sampling return FQL_E_STATE, and fql_group_create with an IFQL
 * member still returns FQL_E_STATE: IFQL handles are grouped by fql_ifql_group_create (below). */
#define FQL_IFQL_NUM_INFO 12
typedef struct fql_ifql_config {
    float expectile;      /* IQL expectile (0.9) */
    int32_t num_samples;  /* best-of-N sample count (32) */
    int32_t reserved[6];
} fql_ifql_config;
void fql_ifql_default_config(fql_ifql_config* c);
int fql_ifql_create(const fql_config* cfg, const fql_ifql_config* icfg, uint64_t seed, fql_handle* out);
/* ---- IFQL agent groups: the seeds of one task, or an expectile x seed sweep, advanced by one fused program (agent groups, above) ----
 * fql_ifql_group_create: `members` [k], k >= 1, IFQL handles (another kind: FQL_E_STATE naming it), distinct, in no group, the same batch
 * size and the same fql_config / fql_ifql_config except expectile (and the create seed); anything else - num_samples, flow_steps, a
 * hidden size, lr - is FQL_E_INVALID naming the member, *out NULL.  The group holds ONE fused program, one graph with a member's lanes:
 * the zip of every member's update (blockIdx.y = member in IFQL's own kernels, concatenated task tables in the layers).  A member's
 * numbers are bitwise those it has alone, and after a group update it behaves as after its own: fql_read_info, its own updates and
 * sampling calls, fql_total_loss, module queries, parameter access and checkpoints.  fql_group_destroy and fql_group_synchronize serve
 * these groups too; fql_set_batch_size and fql_destroy on a member return FQL_E_STATE while it is grouped.  fql_group_create keeps
 * refusing IFQL handles.  Errors: fql_last_error(NULL).
 * Across kinds: the fql_group_*, fql_rebrac_group_* and fql_iqld_group_* calls that take a group return FQL_E_STATE on an IFQL group, and
 * the four calls below that take a group return it on a group of another kind, each naming the call that serves the group; a NULL group
 * is FQL_E_INVALID. */
int fql_ifql_group_create(const fql_handle* members, int k, fql_group* out);
/* fql_update_from_dataset of every member in one fused update.  idx: [k][B] int64, host or device, or NULL = each member's device RNG;
 * x_0 and t are each member's Philox.  info12xk: [k][12] in fql_handle_info_name's order (device or host; host = synchronous) or NULL.
 * Stream and ordering as fql_group_update_from_dataset. */
int fql_ifql_group_update_from_dataset(fql_group g, const int64_t* idx, int batch_size, float* info12xk, void* stream);
/* fql_sample_actions of every member - best of num_samples - in one fused call.  observations [k][n][od], noises
 * [k][n][num_samples][act] or NULL (then seeds [k], each member's Philox), out [k][n][act]; host or device each.  Per chunk of <= 4096
 * sample rows per member (the member's own chunks and row numbers): one repeat launch, the members' Euler flow over concatenated task
 * tables, one critic-input launch, the members' critic pair, one select launch, which writes the actions - 3 launches more than the two
 * programs have, whatever k is.  out[i] is bitwise fql_sample_actions(member i, ..., seeds[i], ...).  Pointer kinds and ordering as
 * fql_group_sample_actions. */
int fql_ifql_group_sample_actions(fql_group g, const float* observations, int n, const float* noises, const uint64_t* seeds, float* out,
                                  void* stream);
/* fql_flow_actions of every member in one fused call: noises [k][n][act], required; everything else as fql_group_flow_actions. */
int fql_ifql_group_flow_actions(fql_group g, const float* observations, const float* noises, int n, float* out, void* stream);
/* Launches of the group's fused update program and of one fused best-of-N call and one fused flow call on a single chunk, counted from
 * the built programs.  Any pointer may be NULL. */
int fql_ifql_group_stats(fql_group g, int64_t* launches_update, int64_t* launches_sample, int64_t* launches_flow);
/* infos per update of this handle: 13 (FQL) or 12 (IFQL); their names, NULL past fql_num_info */
int fql_num_info(fql_handle h);
const char* fql_handle_info_name(fql_handle h, int i);

/* ---- ReBRAC: revisited behavior-regularized actor-critic (agents/rebrac.py), TD3+BC with LayerNorm, on the same engine ----
 * State observations and fp32 only.  Networks (agents/rebrac.py:182-213): "modules_critic/value_net/..." and
 * "modules_target_critic/value_net/..." (FQL's stacked [2, ...] critic), "modules_actor/actor_net/Dense_0..n-1" (+ "LayerNorm_i" with
 * actor_layer_norm) and "modules_actor/mean_net/{bias,kernel}" (utils/networks.py:82-150, const_std: no log-std leaves), and the same
 * under "modules_target_actor".  Glorot-uniform kernels except mean_net's, variance_scaling(actor_fc_scale, fan_avg, uniform); zero
 * biases; both targets are copies at create.
 *
 * Two kinds of update (main.py:207-208): full_update != 0 = critic + actor loss, Adam, Polyak of both targets from the PRE-step critic
 * and actor; full_update == 0 = the critic-only step: the actor's gradient is zero, Adam still runs over every leaf (mu / nu decay, the
 * actor still moves when mu != 0, count and step advance), no Polyak.  Info buffers stay 13 floats:
 *   full step (fql_handle_info_name, 12 keys): 0 critic/critic_loss 1 critic/q_mean 2 critic/q_max 3 critic/q_min 4 actor/total_loss
 *     5 actor/actor_loss 6 actor/bc_loss 7 actor/std 8 actor/mse 9 grad/max 10 grad/min 11 grad/norm; 12 is 0;
 *   critic-only step (7 keys): 0-3 the critic keys, 4 grad/max 5 grad/min 6 grad/norm; 7-12 are 0.
 * The grad statistics run over the whole tree: target leaves, and the actor's on critic-only steps, count with zero gradients.
 * fql_noise: only eps1 is read, the raw N(0, 1) [B, act] of the target-policy noise before actor_noise scaling (agents/rebrac.py:30-34);
 * any other non-NULL pointer is FQL_E_INVALID.  NULL = the engine's Philox stream.
 * next_actions: explicit [B, act] in fql_rebrac_update / fql_rebrac_total_loss; fql_rebrac_update_from_dataset gathers
 * actions[min(idx + 1, size - 1)] with `size` the dataset's current row count (utils/datasets.py:96-100, including its end-of-episode quirk).
 * A ReBRAC handle is an ordinary fql_handle for destroy, set_batch_size, leaf / param / opt-state / step access, dataset upload / add /
 * reserve / size, fql_sample_actions (temperature 1), info enqueue / wait, fql_read_info, fql_synchronize, fql_stats (the full step)
 * and fql_stream.  Refused: encoder != 0 or precision != 0 at create (FQL_E_INVALID); on a ReBRAC handle fql_update,
 * fql_update_from_dataset and fql_total_loss (no next_actions / step kind), fql_update_begin* / _end*, fql_grad_buckets, frame uploads /
 * updates, fql_noise_from_jax_keys, the replay ring, balanced sampling and fql_flow_actions return FQL_E_STATE, and fql_group_create
 * with a ReBRAC member still returns FQL_E_STATE: ReBRAC handles are grouped by fql_rebrac_group_create (below), whose groups hold two
 * fused programs and take the step kind with every update.  The fql_rebrac_* calls on another handle return FQL_E_STATE. */
#define FQL_REBRAC_NUM_INFO 12
#define FQL_REBRAC_CRITIC_NUM_INFO 7
typedef struct fql_rebrac_config {
    float alpha_actor;       /* actor BC coefficient (0.0)                     */
    float alpha_critic;      /* critic BC coefficient (0.0)                    */
    float actor_noise;       /* target-policy / sampling noise scale (0.2)     */
    float actor_noise_clip;  /* noise clip (0.5)                               */
    int32_t tanh_squash;     /* mode = tanh(mean) (1) or mean (0)              */
    float actor_fc_scale;    /* mean_net kernel init scale (0.01)              */
    int32_t reserved[6];
} fql_rebrac_config;
void fql_rebrac_default_config(fql_rebrac_config* c);
int fql_rebrac_create(const fql_config* cfg, const fql_rebrac_config* rcfg, uint64_t seed, fql_handle* out);
/* ReBRACAgent.update(batch, full_update)  agents/rebrac.py:122-134.  info13 as fql_update's (layout above). */
int fql_rebrac_update(fql_handle h, const float* observations, const float* actions, const float* rewards, const float* masks,
                      const float* next_observations, const float* next_actions, int batch_size, const fql_noise* noise,
                      int full_update, float* info13, void* stream);
/* train_dataset.sample(B) + update(batch, full_update) on the device; idx / lo / hi as fql_update_from_dataset's. */
int fql_rebrac_update_from_dataset(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi, const fql_noise* noise,
                                   int full_update, float* info13, void* stream);
/* ReBRACAgent.total_loss(batch, full_update)  agents/rebrac.py:86-108: pure forward, no state change.  loss = critic_loss (+ the actor's
 * total_loss when full_update); info10 receives the first 9 infos of the full layout (4 when !full_update).  Synchronous. */
int fql_rebrac_total_loss(fql_handle h, const float* observations, const float* actions, const float* rewards, const float* masks,
                          const float* next_observations, const float* next_actions, int batch_size, const fql_noise* noise,
                          int full_update, float* loss, float* info10, void* stream);
/* ReBRACAgent.sample_actions(observations, seed, temperature)  agents/rebrac.py:136-152:
 * clip(mode + clip(N(0, 1) actor_noise temperature, +-actor_noise_clip), -1, 1).  noise [n, act] raw N(0, 1) or NULL (engine RNG keyed
 * by `seed`); rows of one call equal single calls with the same noise rows.  fql_sample_actions == this with temperature 1. */
int fql_rebrac_sample_actions(fql_handle h, const float* observations, int n, const float* noise, uint64_t seed, float temperature,
                              float* out, void* stream);
/* launches and algorithmic MACs of one full (full_update != 0) or critic-only update */
int fql_rebrac_stats(fql_handle h, int full_update, int64_t* launches_per_update, int64_t* macs_per_update);
/* ---- ReBRAC agent groups: an alpha_actor x alpha_critic x seed sweep advanced by fused programs (agent groups, above) ----
 * fql_rebrac_group_create: `members` [k], k >= 1, ReBRAC handles (another kind: FQL_E_STATE naming it), distinct, in no group, the same
 * batch size and the same fql_config / fql_rebrac_config except alpha_actor, alpha_critic (and the create seed); anything else:
 * FQL_E_INVALID naming the member, *out NULL.  The group holds TWO fused programs, each one graph with a member's lanes: the zip of
 * every member's full step and the zip of every member's critic-only step (blockIdx.y = member in ReBRAC's own kernels, concatenated
 * task tables in the layers).  A member's numbers are bitwise those it has alone.  fql_group_destroy and fql_group_synchronize serve
 * these groups too; fql_set_batch_size and fql_destroy on a member return FQL_E_STATE while it is grouped.  Errors: fql_last_error(NULL).
 * Across kinds: fql_group_update_from_dataset, fql_group_sample_actions, fql_group_flow_actions and fql_group_sample_stats on a ReBRAC
 * group, and the three calls below that take a group on an FQL group, return FQL_E_STATE; a NULL group is FQL_E_INVALID. */
int fql_rebrac_group_create(const fql_handle* members, int k, fql_group* out);
/* fql_rebrac_update_from_dataset of every member in one fused update, full (full_update != 0) or critic-only.  idx: [k][B] int64, host or
 * device, or NULL = each member's device RNG; next_actions are actions[min(idx + 1, size - 1)] of each member's own dataset.
 * info13xk: [k][13] in fql_rebrac_update's layout for the step's kind (device or host; host = synchronous) or NULL.  Stream and ordering
 * as fql_group_update_from_dataset. */
int fql_rebrac_group_update_from_dataset(fql_group g, const int64_t* idx, int batch_size, int full_update, float* info13xk, void* stream);
/* fql_rebrac_sample_actions of every member in one fused call; shapes, pointer kinds and ordering as fql_group_sample_actions.  Per
 * chunk of <= 4096 rows per member: one assemble launch, the members' actor forward over concatenated task tables, and one launch of
 * ReBRAC's action kernel that writes out[i] directly - the launch count does not depend on k.  out[i] is bitwise
 * fql_rebrac_sample_actions(member i, ..., seeds[i], temperature, ...). */
int fql_rebrac_group_sample_actions(fql_group g, const float* observations, int n, const float* noises, const uint64_t* seeds,
                                    float temperature, float* out, void* stream);
/* Launches of the group's full and critic-only programs and of one fused sampling call on a single chunk, counted from the built
 * programs.  Any pointer may be NULL. */
int fql_rebrac_group_stats(fql_group g, int64_t* launches_full, int64_t* launches_critic, int64_t* launches_sample);

/* ---- SAC (agents/sac.py): soft actor-critic with a squashed Gaussian actor and a learned temperature; RLPD is this agent run online
 * from an empty replay ring with balanced sampling (main.py --offline_steps=0 --balanced_sampling=1).  State observations, fp32 only.
 * Networks (agents/sac.py, utils/networks.py Actor / Value / LogParam): "modules_critic/value_net/..." and
 * "modules_target_critic/value_net/..." (FQL's stacked [2, ...] critic), "modules_actor/actor_net/Dense_0..n-1" (GELU, + "LayerNorm_i"
 * with actor_layer_norm), "modules_actor/mean_net/{bias,kernel}" and "modules_actor/log_std_net/{bias,kernel}" ([H, act] / [act]; kernels
 * variance_scaling(actor_fc_scale, fan_avg, uniform)) and "modules_alpha/log_value" (shape (), initial 0).  Adam over the whole tree,
 * Polyak of the target critic from the PRE-step critic.
 * Infos: 14 floats (FQL_SAC_NUM_INFO, fql_handle_info_name): 0 critic/critic_loss 1 critic/q_mean 2 critic/q_max 3 critic/q_min
 *   4 actor/total_loss 5 actor/actor_loss 6 actor/alpha_loss 7 actor/alpha 8 actor/entropy 9 actor/std 10 actor/q 11 grad/max
 *   12 grad/min 13 grad/norm.  The update calls write 14 floats to info14 (NULL: read later with fql_read_info_n / fql_info_wait_n);
 *   fql_read_info and fql_info_wait return FQL_E_STATE on a SAC handle rather than overrun a 13-float buffer.
 * fql_noise: only eps1 (eps_n: the next-observation actions of the critic loss) and eps2 (eps_c: the actor loss's actions) are read,
 * each the raw N(0, 1) [B, act]; any other non-NULL pointer is FQL_E_INVALID.  NULL = the engine's Philox tensors 1 and 5.
 * A SAC handle is an ordinary fql_handle for destroy, set_batch_size, leaf / param / opt-state / step access, dataset upload / add /
 * reserve / size, replay create / add / size, fql_sample_actions (temperature 1), info enqueue / fql_info_wait_n / fql_read_info_n,
 * fql_synchronize, fql_stats and fql_stream.  Refused: encoder != 0, precision != 0 or state_dependent_std == 0 at create
 * (FQL_E_INVALID); on a SAC handle fql_update*, fql_update_begin* / _end*, fql_total_loss, fql_grad_buckets, frame uploads / updates,
 * fql_noise_from_jax_keys and fql_flow_actions return FQL_E_STATE, and fql_group_create with a SAC member still returns FQL_E_STATE:
 * SAC handles are grouped by fql_sac_group_create (below the CFGRL groups).  The fql_sac_* calls on another handle return FQL_E_STATE. */
#define FQL_SAC_NUM_INFO 14
typedef struct fql_sac_config {
    float target_entropy;             /* NaN = automatic: -target_entropy_multiplier * act_dim (NaN)  */
    float target_entropy_multiplier;  /* (0.5)                                                          */
    int32_t tanh_squash;              /* a = tanh(x) (1) or x (0)                                       */
    int32_t state_dependent_std;      /* log_std_net on the hidden features (1); 0 is refused           */
    float actor_fc_scale;             /* mean_net / log_std_net kernel init scale (0.01)                */
    int32_t backup_entropy;           /* subtract discount mask alpha log_prob' in the target (0)      */
    int32_t reserved[6];
} fql_sac_config;
void fql_sac_default_config(fql_sac_config* c);
/* fql_config.q_agg is read (0 mean, 1 min; SAC's default is min); alpha, flow_steps and normalize_q_loss are ignored. */
int fql_sac_create(const fql_config* cfg, const fql_sac_config* scfg, uint64_t seed, fql_handle* out);
/* SACAgent.update(batch)  agents/sac.py. */
int fql_sac_update(fql_handle h, const float* observations, const float* actions, const float* rewards, const float* masks,
                   const float* next_observations, int batch_size, const fql_noise* noise, float* info14, void* stream);
/* train_dataset.sample(B) + update(batch) on the device; idx / lo / hi as fql_update_from_dataset's. */
int fql_sac_update_from_dataset(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi, const fql_noise* noise,
                                float* info14, void* stream);
/* RLPD's balanced step (main.py:255-259): concat(dataset.sample(B / 2), replay.sample(B / 2)) -> update, gathered on the device.
 * Indices as fql_update_balanced's (both or neither); B must be even; FQL_E_INVALID while the replay ring is empty. */
int fql_sac_update_balanced(fql_handle h, const int64_t* idx_dataset, const int64_t* idx_replay, int batch_size, const fql_noise* noise,
                            float* info14, void* stream);
/* SACAgent.total_loss(batch): pure forward, no state change (parameters, moments, counters and the info slots that fql_read_info_n
 * reads are as the last update left them).  loss = critic_loss + actor total_loss; info11 receives infos 0-10.  Synchronous. */
int fql_sac_total_loss(fql_handle h, const float* observations, const float* actions, const float* rewards, const float* masks,
                       const float* next_observations, int batch_size, const fql_noise* noise, float* loss, float* info11,
                       void* stream);
/* SACAgent.sample_actions(observations, seed, temperature): clip(tanh(mean + exp(log_std) temperature eps), -1, 1) (no tanh when
 * tanh_squash == 0).  noise [n, act] raw N(0, 1) or NULL (engine RNG keyed by `seed`); rows of one call equal single calls with the same
 * noise rows.  fql_sample_actions == this with temperature 1. */
int fql_sac_sample_actions(fql_handle h, const float* observations, int n, const float* noise, uint64_t seed, float temperature,
                           float* out, void* stream);
/* launches and algorithmic MACs of one update */
int fql_sac_stats(fql_handle h, int64_t* launches_per_update, int64_t* macs_per_update);
/* The info calls for any handle: exactly fql_num_info(h) floats into `out` (13 FQL, 12 IFQL / ReBRAC, 14 SAC; nothing past them);
 * FQL_E_INVALID if n < fql_num_info(h). */
int fql_read_info_n(fql_handle h, float* out, int n);
int fql_info_wait_n(fql_handle h, uint64_t ticket, float* out, int n);

/* ---- BC (agents/bc.py): flow-matching behavioural cloning, the baseline agent and the one utils/train.py::train_bc_agent trains.
 * State observations, fp32 only.  One network, a bare TrainState: policy(obs, x_t, emb(t)) = MLP(hidden, GELU, LayerNorm) + Dense(act).
 * Leaves: "MLP_0/Dense_0..n-1/{bias,kernel}" (default_init kernels), "MLP_0/LayerNorm_i/{bias,scale}" with actor_layer_norm, and
 * "Dense_0/{bias,kernel}" (the head: flax's default lecun_normal).  No target network; Adam over the whole tree.
 * fql_config mapping: hidden_dims = actor_hidden / num_actor_hidden, use_layer_norm = actor_layer_norm, bc_lr = lr; the value_* fields,
 * layer_norm, discount, tau, alpha, q_agg, normalize_q_loss and flow_steps are ignored (num_value_hidden must still be in range).
 * Timestep embedding: t = k / S, k in 0..S (S = denoise_steps); emb = [cos(arg_i) | sin(arg_i)], i = 0..7,
 * arg_i = float32(float32(t * 10000) * freq_i), freq_i = float32(exp(-ln(10000) * i / 8) in fp64), cos / sin in fp64 of that fp32
 * argument; the [(S + 1), 16] table is built on the host at create.
 * Infos: 4 floats (FQL_BC_NUM_INFO, fql_handle_info_name): 0 bc_loss 1 grad/max 2 grad/min 3 grad/norm.  The update calls write 4
 * floats to info4 (NULL: read later with fql_read_info_n / fql_info_wait_n); fql_read_info and fql_info_wait return FQL_E_STATE.
 * fql_noise: only x0 [B, act] (raw N(0, 1)) and t [B] are read; t must lie on the grid {0, 1/S, ..., 1} and is read as round(t S)
 * (a host t off the grid is FQL_E_INVALID); any other non-NULL pointer is FQL_E_INVALID.  NULL = the engine's Philox tensors 2 and 3.
 * A BC handle is an ordinary fql_handle for destroy, set_batch_size, leaf / param / opt-state / step access, dataset upload / add /
 * reserve / size, info enqueue / fql_info_wait_n / fql_read_info_n, fql_synchronize, fql_stats and fql_stream.  Refused: encoder != 0
 * or precision != 0 at create (FQL_E_INVALID); on a BC handle fql_update*, fql_update_begin* / _end*, fql_total_loss,
 * fql_sample_actions, fql_flow_actions, fql_grad_buckets, frame uploads / updates, fql_replay_*, fql_update_balanced,
 * fql_noise_from_jax_keys, fql_read_info, fql_info_wait and every fql_rebrac_* / fql_sac_* call return FQL_E_STATE, and
 * fql_group_create with a BC member returns FQL_E_STATE.  The fql_bc_* calls on another handle return FQL_E_STATE. */
#define FQL_BC_NUM_INFO 4
typedef struct fql_bc_config {
    int32_t denoise_steps;            /* S: grid of t and Euler steps of sample_actions (16) */
    int32_t reserved[7];
} fql_bc_config;
void fql_bc_default_config(fql_bc_config* c);
int fql_bc_create(const fql_config* cfg, const fql_bc_config* bcfg, uint64_t seed, fql_handle* out);
/* BCAgent.update(batch)  agents/bc.py:72-84: observations [B, obs], actions [B, act]. */
int fql_bc_update(fql_handle h, const float* observations, const float* actions, int batch_size, const fql_noise* noise, float* info4,
                  void* stream);
/* train_dataset.sample(B) + update(batch) on the device; idx / lo / hi as fql_update_from_dataset's. */
int fql_bc_update_from_dataset(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi, const fql_noise* noise,
                               float* info4, void* stream);
/* BCAgent.policy_loss(batch): pure forward, no state change (parameters, moments, counters and the info slots that fql_read_info_n
 * reads are as the last update left them).  Synchronous. */
int fql_bc_policy_loss(fql_handle h, const float* observations, const float* actions, int batch_size, const fql_noise* noise, float* loss,
                       void* stream);
/* BCAgent.sample_actions(observations, seed): x ~ N(0, I); S times x += policy(obs, x, i / S) / S; clip to [-1, 1].  noise [n, act] or
 * NULL (engine RNG keyed by `seed`); rows of one call equal single calls with the same noise rows. */
int fql_bc_sample_actions(fql_handle h, const float* observations, int n, const float* noise, uint64_t seed, float* out, void* stream);
/* launches and algorithmic MACs of one update; launches of one sampling call of <= 4096 rows */
int fql_bc_stats(fql_handle h, int64_t* launches_per_update, int64_t* macs_per_update, int64_t* launches_per_sample);

/* ---- IQL (agents/iql.py): implicit Q-learning, the classic offline baseline.  State observations, fp32 only.
 * Networks (utils/networks.py Value / Actor): "modules_value/value_net/..." (one member, unstacked), "modules_critic/value_net/..." and
 * "modules_target_critic/value_net/..." (FQL's stacked [2, ...] critic), "modules_actor/actor_net/Dense_0..n-1" (GELU, + "LayerNorm_i"
 * with actor_layer_norm), "modules_actor/mean_net/{bias,kernel}" ([H, act] / [act], kernel variance_scaling(1e-2, fan_avg, uniform)) and,
 * with const_std == 0 only, "modules_actor/log_stds" ([act], zeros, clipped to [-5, 2] where it is read).  A plain Gaussian: no tanh.
 * Adam over the whole tree, Polyak of the target critic from the PRE-step critic.
 * Losses: the value and critic losses are IFQL's (expectile regression onto min of the target pair at (obs, act); TD onto
 * value(next_obs)).  Actor, actor_loss == 0 (awr): -mean(min(exp(alpha (min(q1, q2) - v)), 100) log_prob(actions)), the weight a
 * constant; actor_loss == 1 (ddpgbc): a = clip(mean) (const_std) or clip(mean + exp(log_stds) eps), -mean(min(q1, q2)(obs, a)) /
 * stop_gradient(mean |q|) - alpha mean(log_prob(actions)); minimum and clip pass 1/2 of the gradient at an exact tie / bound.
 * Infos (fql_num_info, fql_handle_info_name): 0 value/value_loss 1 value/v_mean 2 value/v_max 3 value/v_min 4 critic/critic_loss
 *   5 critic/q_mean 6 critic/q_max 7 critic/q_min, then
 *   awr (16, FQL_IQL_AWR_NUM_INFO):       8 actor/actor_loss 9 actor/adv 10 actor/bc_log_prob 11 actor/mse 12 actor/std 13 grad/max
 *                                         14 grad/min 15 grad/norm
 *   ddpgbc (19, FQL_IQL_DDPGBC_NUM_INFO): 8 actor/actor_loss 9 actor/q_loss 10 actor/bc_loss 11 actor/q_mean 12 actor/q_abs_mean
 *                                         13 actor/bc_log_prob 14 actor/mse 15 actor/std 16 grad/max 17 grad/min 18 grad/norm
 *   The update calls write fql_num_info(h) floats to `info` (NULL: read later with fql_read_info_n / fql_info_wait_n); fql_read_info and
 *   fql_info_wait return FQL_E_STATE on an IQL handle rather than overrun a 13-float buffer.
 * fql_noise: only eps1 (the raw N(0, 1) [B, act] of dist.sample in ddpgbc with const_std == 0; ignored otherwise) is read; any other
 * non-NULL pointer is FQL_E_INVALID.  NULL = the engine's Philox tensor 1.
 * An IQL handle is an ordinary fql_handle for destroy, set_batch_size, leaf / param / opt-state / step access, dataset upload / add /
 * reserve / size, fql_sample_actions (temperature 1), info enqueue / fql_info_wait_n / fql_read_info_n, fql_synchronize, fql_stats and
 * fql_stream.  Refused: encoder != 0 or precision != 0 at create (FQL_E_INVALID); on an IQL handle fql_update*, fql_update_begin* /
 * _end*, fql_total_loss, fql_flow_actions, fql_grad_buckets, frame uploads / updates, fql_replay_*, fql_update_balanced,
 * fql_noise_from_jax_keys, fql_read_info and fql_info_wait return FQL_E_STATE, and fql_group_create with an IQL member still returns
 * FQL_E_STATE: IQL handles are grouped by fql_iql_group_create (below).  The fql_iql_* calls on another handle return FQL_E_STATE. */
#define FQL_IQL_AWR_NUM_INFO 16
#define FQL_IQL_DDPGBC_NUM_INFO 19
typedef struct fql_iql_config {
    float expectile;                  /* IQL expectile, in (0, 1) (0.9)                               */
    float alpha;                      /* temperature in AWR / BC coefficient in DDPG+BC (1.0)          */
    int32_t actor_loss;               /* 0 = awr, 1 = ddpgbc (1)                                       */
    int32_t const_std;                /* 1: log-std 0, no log_stds leaf; 0: the learned vector (1)     */
    int32_t reserved[8];
} fql_iql_config;
void fql_iql_default_config(fql_iql_config* c);
/* fql_config.alpha, q_agg, flow_steps and normalize_q_loss are ignored (alpha is fql_iql_config's). */
int fql_iql_create(const fql_config* cfg, const fql_iql_config* qcfg, uint64_t seed, fql_handle* out);
/* IQLAgent.update(batch)  agents/iql.py:145-156. */
int fql_iql_update(fql_handle h, const float* observations, const float* actions, const float* rewards, const float* masks,
                   const float* next_observations, int batch_size, const fql_noise* noise, float* info, void* stream);
/* train_dataset.sample(B) + update(batch) on the device; idx / lo / hi as fql_update_from_dataset's. */
int fql_iql_update_from_dataset(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi, const fql_noise* noise,
                                float* info, void* stream);
/* IQLAgent.total_loss(batch): pure forward, no state change (parameters, moments, counters and the infos that fql_read_info_n reads are
 * as the last update left them).  loss = value_loss + critic_loss + actor_loss; `info` receives the fql_num_info(h) - 3 infos before the
 * grad statistics.  Synchronous. */
int fql_iql_total_loss(fql_handle h, const float* observations, const float* actions, const float* rewards, const float* masks,
                       const float* next_observations, int batch_size, const fql_noise* noise, float* loss, float* info, void* stream);
/* IQLAgent.sample_actions(observations, seed, temperature): clip(mean + exp(log_stds) temperature eps, -1, 1); temperature 0 returns
 * clip(mean) exactly.  noise [n, act] raw N(0, 1) or NULL (engine RNG keyed by `seed`); rows of one call equal single calls with the same
 * noise rows.  fql_sample_actions == this with temperature 1. */
int fql_iql_sample_actions(fql_handle h, const float* observations, int n, const float* noise, uint64_t seed, float temperature,
                           float* out, void* stream);
/* launches and algorithmic MACs of one update */
int fql_iql_stats(fql_handle h, int64_t* launches_per_update, int64_t* macs_per_update);
/* ---- IQL agent groups: the seeds of one task, or an alpha x expectile x seed sweep, advanced by one fused program (agent groups, above) ----
 * fql_iql_group_create: `members` [k], k >= 1, IQL handles (another kind: FQL_E_STATE naming it), distinct, in no group, the same batch
 * size and the same fql_config / fql_iql_config except expectile and alpha (and the create seed); anything else - actor_loss, const_std,
 * a hidden size, lr - is FQL_E_INVALID naming the member, *out NULL.  The group holds ONE fused program, one graph with a member's lanes:
 * the zip of every member's update (blockIdx.y = member in IQL's own kernels and in IFQL's two losses, concatenated task tables in the
 * layers), a member's launch count whatever k is.  A member's numbers are bitwise those it has alone, and after a group update it behaves
 * as after its own: fql_read_info_n (its own 16 or 19 infos), its own updates and sampling calls, fql_iql_total_loss, parameter access
 * and checkpoints.  fql_group_destroy and fql_group_synchronize serve these groups too; fql_set_batch_size and fql_destroy on a member
 * return FQL_E_STATE while it is grouped.  fql_group_create and the other kinds' creates keep refusing IQL handles.  Errors:
 * fql_last_error(NULL).
 * Across kinds: the fql_group_*, fql_rebrac_group_*, fql_iqld_group_* and fql_ifql_group_* calls that take a group return FQL_E_STATE on
 * an IQL group, and the three calls below that take a group return it on a group of another kind, each naming the call that serves the
 * group; a NULL group is FQL_E_INVALID. */
int fql_iql_group_create(const fql_handle* members, int k, fql_group* out);
/* fql_iql_update_from_dataset of every member in one fused update.  idx: [k][B] int64, host or device, or NULL = each member's device
 * RNG; eps is each member's Philox.  infoNxk: [k][fql_num_info] - 16 (awr) or 19 (ddpgbc) per member, as fql_read_info_n gives them -
 * device or host (host = synchronous), or NULL.  Stream and ordering as fql_group_update_from_dataset. */
int fql_iql_group_update_from_dataset(fql_group g, const int64_t* idx, int batch_size, float* infoNxk, void* stream);
/* fql_iql_sample_actions of every member in one fused call.  observations [k][n][od], noises [k][n][act] raw N(0, 1) or NULL (then seeds
 * [k], each member's Philox keyed by its own seed and the row's number in the call), one temperature for the call, out [k][n][act]; host
 * or device each.  Per chunk of <= 4096 rows per member: one assemble launch, the members' actor over concatenated task tables, one
 * sampling-head launch with each member's own log_stds, which writes the actions - 2 launches more than the actor has layers, whatever k
 * is.  out[i] is bitwise fql_iql_sample_actions(member i, ..., seeds[i], temperature, ...).  Pointer kinds and ordering as
 * fql_group_sample_actions. */
int fql_iql_group_sample_actions(fql_group g, const float* observations, int n, const float* noises, const uint64_t* seeds,
                                 float temperature, float* out, void* stream);
/* Launches of the group's fused update program and of one fused sampling call on a single chunk, counted from the built programs.
 * Either pointer may be NULL. */
int fql_iql_group_stats(fql_group g, int64_t* launches_update, int64_t* launches_sample);

/* ---- IQL-diffusion (agents/iql_diffusion.py): IQL critics with an optimality-conditioned flow actor and classifier-free guidance, the
 * agent the CFGRL training script defaults to.  The BINARY optimality family only: optimal_var in {binary, binary_awr_loss,
 * binary_softmax_loss}, whose actor is DiffusionPolicy with nn.Embed(2, 32).  State observations, fp32, GELU, a constant learning rate.
 * Four bare TrainStates (no ModuleDict), leaves in jax dict order:
 *   "actor/Dense_0/{bias,kernel}" (the head, flax's lecun_normal), "actor/Embed_0/embedding" ([2, 32], N(0, 1 / 32): flax's
 *   variance_scaling(1, fan_in, normal, out_axis=0), whose fan_in on [2, 32] is 32), "actor/MLP_0/Dense_i/{bias,kernel}" (first layer
 *   obs + act + 16 + 32 -> hidden) and "actor/MLP_0/LayerNorm_i/{bias,scale}" with actor_layer_norm;
 *   "critic/value_net/..." and "target_critic/value_net/..." (stacked [2, ...]), "value/value_net/..." (one member, unstacked).
 * fql_config mapping: actor_hidden = actor_hidden_dims, value_hidden = hidden_dims, layer_norm = actor_layer_norm = use_layer_norm;
 * lr, alpha, q_agg, flow_steps and normalize_q_loss are ignored (the three learning rates travel in fql_iqld_config).
 * Update (agents/iql_diffusion.py:215-247), the reference's static flags as arguments: update_critic steps the critic (Adam critic_lr,
 * Polyak of the target from the PRE-step critic) and the value net (Adam value_lr); update_actor steps the actor (Adam actor_lr).  Each
 * TrainState keeps its own Adam count: a step kind leaves the other nets' parameters, moments and counts untouched; (0, 0) changes no
 * parameter and still advances the RNG step.  Losses: value = expectile regression onto min of the target pair at (obs, act); critic =
 * mean over BOTH members and the batch of (q_e - r - discount mask v(next_obs))^2 (half of agents/iql.py's); actor = mean_b(w_b
 * mean_a((vel - v_pos)^2) + 0.1 mean_a((vel - v_unc)^2)) with the weights w from adv = min(q1, q2)(obs, act) - v(obs) on stored
 * parameters (the target pair with target_extraction, else the critic): binary adv > 0; binary_awr_loss min(where(adv > 0,
 * clip(exp(adv awr_temperature), 0, 1e8), 0), 100); binary_softmax_loss e / (sum e + 1e-8), e = where(adv > 0, clip(exp(adv
 * softmax_beta), 0, 1e8), 0).
 * Infos: 21 floats (FQL_IQLD_NUM_INFO, fql_handle_info_name): 0 critic_loss 1 q (member 0's mean) 2 value_loss 3 v 4 v_min 5 v_max
 *   6 actor_q 7 actor_loss 8 actor_positive_ratio 9 actor_loss_positive 10 actor_loss_uncond 11 o_mean 12 o_std 13 o_min 14 o_max
 *   15 effective_batch_size 16 loss_weights_top_10_mass 17 loss_weights_max 18 grad/max 19 grad/min 20 grad/norm.  The reference merges
 *   {**critic_info, **value_info, **actor_info}: grad/... are the ACTOR's gradient statistics when update_actor, otherwise the value
 *   net's, never the critic's.  The slots of a net that did not step are 0.  fql_read_info and fql_info_wait return FQL_E_STATE.
 * fql_noise: only x0 [B, act] (raw N(0, 1)) and t [B] on the grid {0, 1/S, ..., 1} are read, as on a BC handle.
 * An IQL-diffusion handle is an ordinary fql_handle for destroy, set_batch_size, leaf / param / opt-state access, dataset upload / add /
 * reserve / size, info enqueue / fql_info_wait_n / fql_read_info_n, fql_synchronize, fql_stats (the full step) and fql_stream;
 * fql_get_step reads the critic's count and step (fql_iqld_get_steps reads all three counters).  Refused: at create, FQL_E_INVALID
 * naming the field: optimal_var softmax / sampled_adv_softmax (the continuous policy with an external bc_agent), opt_decay_schedule
 * cosine, encoder != 0, precision != 0.  On an IQL-diffusion handle fql_update*, fql_update_begin* / _end*, fql_total_loss,
 * fql_sample_actions, fql_flow_actions, fql_grad_buckets, frame uploads / updates, fql_replay_*, fql_update_balanced,
 * fql_noise_from_jax_keys, fql_read_info, fql_info_wait, fql_set_step (fql_iqld_set_steps writes both counter blocks), fql_set_grad_scale
 * and every other kind's calls return FQL_E_STATE, and fql_group_create with such a
 * member still returns FQL_E_STATE: IQL-diffusion handles are grouped by fql_iqld_group_create (below), whose groups hold one fused
 * program per step kind.  The fql_iqld_* calls on another handle return FQL_E_STATE. */
#define FQL_IQLD_NUM_INFO 21
typedef struct fql_iqld_config {
    float actor_lr, value_lr, critic_lr;  /* 3e-4 each                                                          */
    float expectile;                      /* 0.9                                                                */
    float awr_temperature;                /* 0.1                                                                */
    float softmax_beta;                   /* 3.0                                                                */
    int32_t optimal_var;                  /* 0 binary, 1 binary_awr_loss (default), 2 binary_softmax_loss; 3 softmax and
                                             4 sampled_adv_softmax are refused                                  */
    int32_t target_extraction;            /* adv from the target critic (1) or the critic (0)                   */
    int32_t denoise_steps;                /* S: grid of t and Euler steps of sample_actions (16)                */
    int32_t opt_decay_schedule;           /* 0 none; 1 cosine is refused                                        */
    int32_t reserved[6];
} fql_iqld_config;
void fql_iqld_default_config(fql_iqld_config* c);
int fql_iqld_create(const fql_config* cfg, const fql_iqld_config* dcfg, uint64_t seed, fql_handle* out);
/* IQLDiffusionAgent.update(batch, update_critic, update_actor).  `info`: 21 floats, or NULL. */
int fql_iqld_update(fql_handle h, const float* observations, const float* actions, const float* rewards, const float* masks,
                    const float* next_observations, int batch_size, const fql_noise* noise, int update_critic, int update_actor,
                    float* info, void* stream);
/* train_dataset.sample(B) + update(batch, ...) on the device; idx / lo / hi as fql_update_from_dataset's. */
int fql_iqld_update_from_dataset(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi, const fql_noise* noise,
                                 int update_critic, int update_actor, float* info, void* stream);
/* IQLDiffusionAgent.total_loss(batch): pure forward, no state change (parameters, moments, counters, and what fql_read_info_n and
 * fql_iqld_read_rows(0..2) read are as the last update left them).  loss = critic_loss + value_loss + actor_loss; `info`
 * receives the 18 infos before the grad statistics.  Synchronous. */
int fql_iqld_total_loss(fql_handle h, const float* observations, const float* actions, const float* rewards, const float* masks,
                        const float* next_observations, int batch_size, const fql_noise* noise, float* loss, float* info, void* stream);
/* IQLDiffusionAgent.sample_actions(observations, seed, temperature, cfg, o): x ~ N(0, I); S times v = v_unc + cfg (v_pos - v_unc),
 * x += v / S; clip to [-1, 1].  temperature and o are not read in this family.  noise [n, act] or NULL (engine RNG keyed by `seed`);
 * rows of one call equal single calls with the same noise rows. */
int fql_iqld_sample_actions(fql_handle h, const float* observations, int n, const float* noise, uint64_t seed, float cfg, float* out,
                            void* stream);
/* The per-row infos of the last actor step: which = 0 actor_losses, 1 o (all ones), 2 loss_weights; 3, 4, 5: the same of the last
 * fql_iqld_total_loss.  n = the batch size; `out` host.  Synchronous. */
int fql_iqld_read_rows(fql_handle h, int which, float* out, int n);
/* [0] updates so far (the RNG step), [1] the critic's and value net's Adam count, [2] the actor's; TrainState.step is count + 1.
 * fql_iqld_set_steps restores them (a checkpoint): the next update draws what the saved agent would have drawn. */
int fql_iqld_get_steps(fql_handle h, int64_t steps[3]);
int fql_iqld_set_steps(fql_handle h, const int64_t steps[3]);
/* launches and algorithmic MACs of one update of that step kind; launches of one sampling call of <= 2048 observations */
int fql_iqld_stats(fql_handle h, int update_critic, int update_actor, int64_t* launches_per_update, int64_t* macs_per_update,
                   int64_t* launches_per_sample);
/* ---- IQL-diffusion agent groups: a softmax_beta / awr_temperature x seed sweep advanced by fused programs (agent groups, above) ----
 * fql_iqld_group_create: `members` [k], k >= 1, IQL-diffusion handles (another kind: FQL_E_STATE naming it), distinct, in no group, the
 * same batch size and the same fql_config / fql_iqld_config except awr_temperature, softmax_beta (and the create seed); anything else -
 * optimal_var, expectile, target_extraction, a learning rate, a hidden size - is FQL_E_INVALID naming the member, *out NULL.  The group
 * holds FOUR fused programs, each one graph with a member's lanes: the zip of every member's program of one step kind (full, critic-only,
 * actor-only, neither; blockIdx.y = member in the agent's own kernels, concatenated task tables in the layers).  A member's numbers are
 * bitwise those it has alone, and after a group update it behaves as after its own: fql_iqld_read_rows, fql_iqld_get_steps,
 * fql_read_info_n, its own updates and sampling calls, module queries and checkpoints.  fql_group_destroy and fql_group_synchronize serve
 * these groups too; fql_set_batch_size and fql_destroy on a member return FQL_E_STATE while it is grouped.  fql_group_create keeps
 * refusing IQL-diffusion handles.  Errors: fql_last_error(NULL).
 * Across kinds: the fql_group_* and fql_rebrac_group_* calls that take a group return FQL_E_STATE on an IQL-diffusion group, and the three
 * calls below that take a group return it on an FQL or ReBRAC group, each naming the call that serves the group; a NULL group is
 * FQL_E_INVALID. */
int fql_iqld_group_create(const fql_handle* members, int k, fql_group* out);
/* fql_iqld_update_from_dataset of every member in one fused update of the step kind (update_critic, update_actor).  idx: [k][B] int64,
 * host or device, or NULL = each member's device RNG; x_0 and t are each member's Philox.  info21xk: [k][21] in fql_read_info_n's layout
 * (the slots of a net that did not step are 0; device or host; host = synchronous) or NULL.  Every step kind advances each member's
 * update counter, and only the Adam counts that kind advances alone; (0, 0) moves the RNG step and nothing else.  Stream and ordering
 * as fql_group_update_from_dataset. */
int fql_iqld_group_update_from_dataset(fql_group g, const int64_t* idx, int batch_size, int update_critic, int update_actor,
                                       float* info21xk, void* stream);
/* fql_iqld_sample_actions_cfgs of every member in one fused call.  observations [k][n][od], noises [k][n][act] or NULL (then seeds [k],
 * each member's Philox), cfgs [k][n] (one guidance weight per member and row: a scalar cfg or one per member is that value repeated;
 * host: every weight finite, else FQL_E_INVALID; or device), out [k][n][act]; host or device each.  Per chunk of <= 2048 observations
 * per member: one assemble launch, the members' sweep program over concatenated task tables and [k] argument structs, one extract
 * launch - the launch count of fql_sample_cfgs_stats, whatever k is.  out[i] is bitwise
 * fql_iqld_sample_actions_cfgs(member i, ..., seeds[i], cfgs[i], ...), whose row j is fql_iqld_sample_actions at cfg = cfgs[i][j].
 * Pointer kinds and ordering as fql_group_sample_actions. */
int fql_iqld_group_sample_actions(fql_group g, const float* observations, int n, const float* noises, const uint64_t* seeds,
                                  const float* cfgs, float* out, void* stream);
/* Launches of the group's four programs - [0] full, [1] critic-only, [2] actor-only, [3] neither - and of one fused sampling call on a
 * single chunk, counted from the built programs.  Either pointer may be NULL. */
int fql_iqld_group_stats(fql_group g, int64_t launches[4], int64_t* launches_sample);

/* ---- CFGRL (agents/cfgrl.py): classifier-free-guidance RL, a goal-conditioned flow policy.  State observations, fp32, GELU.
 * One ModuleDict TrainState (`network`), leaves in jax dict order:
 *   "modules_actor_flow/mlp/Dense_i/{bias,kernel}" (GCActorVectorField: MLP((*actor_hidden, act)) on [obs | goals | x_t | t], first layer
 *   obs + goal_dim + act + 1 -> hidden, every kernel Glorot uniform) and "modules_actor_flow/mlp/LayerNorm_i/{bias,scale}" with
 *   actor_layer_norm; "modules_unc_embed/Embed_0/embedding" ([1, goal_dim], N(0, 1 / goal_dim): flax's variance_scaling(1, fan_in,
 *   normal, out_axis=0), whose fan_in on [1, G] is G).
 * fql_config mapping: actor_hidden = actor_hidden_dims, actor_layer_norm, lr; value_hidden, layer_norm, discount, tau, alpha, q_agg,
 * flow_steps and normalize_q_loss are ignored (flow_steps travels in fql_cfgrl_config).
 * Update (agents/cfgrl.py:22-68): x_0 ~ N(0, I), t ~ U[0, 1), x_t = (1 - t) x_0 + t a, vel = a - x_0; do_cfg ~ Bernoulli(p_uncond) per
 * row; goals = where(do_cfg, unc_embed, actor_goals); loss = mean((actor_flow(obs, x_t, t, goals) - vel)^2) over B act elements.  The
 * gradient reaches unc_embed through the dropped rows only.  Adam over the whole tree, no target network.
 * Infos: 4 floats (FQL_CFGRL_NUM_INFO, fql_handle_info_name): 0 actor/actor_loss 1 grad/max 2 grad/min 3 grad/norm; fql_read_info and
 * fql_info_wait return FQL_E_STATE.
 * fql_noise: only x0 [B, act] (raw N(0, 1)) and t [B] in [0, 1) are read; any other non-NULL pointer is FQL_E_INVALID.  do_cfg: [B]
 * bytes (non-zero = the row's goal is dropped), host or device, or NULL = u32 < floor(p_uncond 2^32) of a Philox tensor of its own.
 * Goals on the device (utils/datasets.py:224-255, GCDataset.sample_goals with the actor's probabilities): fql_cfgrl_dataset_goals stores
 * the per-row `final` table beside the uploaded dataset; fql_cfgrl_update_from_dataset then draws, per row, idx, a random goal, d, u and
 * u' (32 bits each, u32 / 2^32 as a double) and takes round(min(idx + 1, final) d + final (1 - d)) in fp64 (each operation rounded on
 * its own, half to even), where(u < p_traj / (1 - p_cur), ., random), where(u' < p_cur, idx, .); p_cur == 1: goal = idx.
 * A CFGRL handle is an ordinary fql_handle for destroy, set_batch_size, leaf / param / opt-state / step access, dataset upload / reserve /
 * size, info enqueue / fql_info_wait_n / fql_read_info_n, fql_synchronize, fql_stats and fql_stream; fql_dataset_upload and
 * fql_dataset_add drop the goal table.  Refused: at create, FQL_E_INVALID naming the field: actor_geom_sample != 0, encoder != 0,
 * precision != 0, goal_dim outside [1, 1024], probabilities that do not sum to 1.  On a CFGRL handle fql_update*, fql_update_begin* /
 * _end*, fql_total_loss, fql_sample_actions, fql_flow_actions, fql_grad_buckets, frame uploads / updates, fql_replay_*,
 * fql_update_balanced, fql_noise_from_jax_keys, fql_read_info, fql_info_wait and every other kind's calls return FQL_E_STATE, and
 * fql_group_create with such a member still returns FQL_E_STATE: CFGRL handles are grouped by fql_cfgrl_group_create (below the guidance
 * sweeps).  The fql_cfgrl_* calls on another handle return FQL_E_STATE. */
#define FQL_CFGRL_NUM_INFO 4
typedef struct fql_cfgrl_config {
    int32_t goal_dim;                 /* G: last axis of example_batch['value_goals']; need not equal obs_dim   */
    int32_t flow_steps;               /* Euler steps of sample_actions (16)                                     */
    float cfg;                        /* the guidance scale the host mirror passes by default (3.0)             */
    int32_t actor_geom_sample;        /* 0; 1 is refused                                                        */
    double p_uncond;                  /* probability that a row's goal is replaced by unc_embed (0.1)           */
    double actor_p_curgoal;           /* 0.0                                                                    */
    double actor_p_trajgoal;          /* 1.0                                                                    */
    double actor_p_randomgoal;        /* 0.0                                                                    */
    int32_t reserved[6];
} fql_cfgrl_config;
void fql_cfgrl_default_config(fql_cfgrl_config* c);
int fql_cfgrl_create(const fql_config* cfg, const fql_cfgrl_config* gcfg, uint64_t seed, fql_handle* out);
/* CFGRLAgent.update(batch): observations [B, obs], actions [B, act], actor_goals [B, goal_dim].  `info4`: 4 floats, or NULL. */
int fql_cfgrl_update(fql_handle h, const float* observations, const float* actions, const float* actor_goals, int batch_size,
                     const fql_noise* noise, const uint8_t* do_cfg, float* info4, void* stream);
/* The per-row `final` table (int64 [N]: the last row of row i's trajectory, terminal_locs[searchsorted(terminal_locs, i)]) and the goal
 * representations (float [N, goal_dim], or NULL: the observations, which needs goal_dim == obs_dim) of the uploaded dataset. */
int fql_cfgrl_dataset_goals(fql_handle h, const int64_t* final_idx, const float* reps);
/* GCDataset.sample(B) + update(batch) on the device; idx / lo / hi as fql_update_from_dataset's.  FQL_E_INVALID without the goal table. */
int fql_cfgrl_update_from_dataset(fql_handle h, const int64_t* idx, int batch_size, int64_t lo, int64_t hi, const fql_noise* noise,
                                  const uint8_t* do_cfg, float* info4, void* stream);
/* actor_loss with the stored parameters: pure forward, no state change (parameters, moments, counters, and what fql_read_info_n and
 * fql_cfgrl_read_rows(probe = 0) read are as the last update left them).  Synchronous. */
int fql_cfgrl_policy_loss(fql_handle h, const float* observations, const float* actions, const float* actor_goals, int batch_size,
                          const fql_noise* noise, const uint8_t* do_cfg, float* loss, void* stream);
/* CFGRLAgent.sample_actions(observations, goals, seed): x ~ N(0, I); flow_steps times v = v_unc + cfg (v_cond - v_unc) at t = i /
 * flow_steps, x += v / flow_steps; clip to [-1, 1].  goals [n, goal_dim]: NULL is FQL_E_INVALID.  noise [n, act] or NULL (engine RNG
 * keyed by `seed` and the row number); rows of one call equal single calls with the same noise rows. */
int fql_cfgrl_sample_actions(fql_handle h, const float* observations, const float* goals, int n, const float* noise, uint64_t seed,
                             float cfg, float* out, void* stream);
/* The rows of the last update (probe = 0) or the last fql_cfgrl_policy_loss (probe = 1); every pointer host, NULL = not wanted:
 * idx [n], goal_idx [n] (-1: the goals came with the batch), do_cfg [n], draws [6][n] (the raw 32-bit draws: idx, random goal, d, u, u',
 * mask; 0 where none was made), goals [n, goal_dim] (the goal columns of the input rows as assembled, whichever call ran last).
 * n = the batch size.  Synchronous. */
int fql_cfgrl_read_rows(fql_handle h, int probe, int64_t* idx, int64_t* goal_idx, uint8_t* do_cfg, uint32_t* draws, float* goals, int n);
/* launches and algorithmic MACs of one update; launches of one sampling call of <= 2048 observations */
int fql_cfgrl_stats(fql_handle h, int64_t* launches_per_update, int64_t* macs_per_update, int64_t* launches_per_sample);

/* ---- Guidance sweeps: the two classifier-free-guidance samplers with ONE WEIGHT PER ROW, so that one call serves every weight of an
 * evaluation sweep (main.py:298-330 evaluates cfg in [1, 1.5, 3, 5], one rollout each) or several vector envs stepped in lockstep.
 * cfgs: [n] floats, host or device.  Row j of the result is, bit for bit, row j of fql_iqld_sample_actions / fql_cfgrl_sample_actions
 * called with cfg = cfgs[j] on the same observation (goal), noise row and, with engine noise, the same seed and row number.  The call
 * runs a program of its own (S - 1 launches fewer: the guidance step of Euler step i - 1 runs inside the first launch of step i); the
 * scalar calls above, their launches and their results are untouched.
 * FQL_E_INVALID: cfgs == NULL, n <= 0, a non-finite weight in a host array (fql_last_error names the row; a device array is not read on
 * the host), goals == NULL on CFGRL.  FQL_E_STATE: a handle of another kind. */
int fql_iqld_sample_actions_cfgs(fql_handle h, const float* observations, int n, const float* noise, uint64_t seed,
                                 const float* cfgs /* [n] */, float* out, void* stream);
int fql_cfgrl_sample_actions_cfgs(fql_handle h, const float* observations, const float* goals, int n, const float* noise,
                                  uint64_t seed, const float* cfgs /* [n] */, float* out, void* stream);
/* launches of one such call of <= 2048 rows, counted from the built program: 4 + S nl + 1 (IQL-diffusion), 3 + S nl + 1 (CFGRL), where
 * fql_iqld_stats / fql_cfgrl_stats report 4 + S (nl + 1) / 3 + S (nl + 1) for the scalar call.  IQL-diffusion and CFGRL handles only. */
int fql_sample_cfgs_stats(fql_handle h, int64_t* launches_per_call);

/* ---- CFGRL agent groups: a seed x goal-mixture x guidance-weight sweep advanced by one fused program (agent groups, above) ----
 * fql_cfgrl_group_create: `members` [k], k >= 1, CFGRL handles (another kind: FQL_E_STATE naming it), distinct, in no group, the same
 * batch size and the same fql_config / fql_cfgrl_config except cfg, actor_p_curgoal, actor_p_trajgoal, actor_p_randomgoal (and the create
 * seed); anything else - goal_dim, flow_steps, p_uncond, actor_layer_norm, a hidden size, lr - is FQL_E_INVALID naming the member and
 * the fields that may differ, *out NULL.  cfg is the default guidance weight, an argument of the sampling calls; the three probabilities
 * reach the device only through each member's goal source, which every update writes.  The group holds ONE fused program, one graph on a
 * member's single lane: the zip of every member's update (blockIdx.y = member in CFGRL's own kernels, concatenated task tables in the
 * layers, the weight gradients and Adam).  A member's numbers are bitwise those it has alone, and after a group update it behaves as
 * after its own: fql_cfgrl_read_rows(probe = 0), fql_read_info_n, fql_cfgrl_policy_loss, its own updates and sampling calls, parameter
 * access and checkpoints.  fql_group_destroy and fql_group_synchronize serve these groups too; fql_set_batch_size and fql_destroy on a
 * member return FQL_E_STATE while it is grouped.  fql_group_create and the other kinds' group creates keep refusing CFGRL handles and name
 * this call.  Errors: fql_last_error(NULL).
 * Across kinds: every other kind's call that takes a group returns FQL_E_STATE on a CFGRL group, and the three calls below that take a
 * group return it on a group of another kind, each naming the call that serves the group; a NULL group is FQL_E_INVALID. */
int fql_cfgrl_group_create(const fql_handle* members, int k, fql_group* out);
/* fql_cfgrl_update_from_dataset of every member in one fused update.  idx: [k][B] int64, host or device, or NULL = each member's device
 * RNG.  do_cfg: [k][B] bytes (non-zero = the row's goal is dropped), host or device, or NULL = each member's own Philox mask.  Per
 * member the call sets the dataset source and the goal source - its goal table (required: without one FQL_E_INVALID naming the member),
 * its mixture thresholds, its rows of do_cfg - then launches the one graph.  x_0, t, the index draw and the four goal draws are each
 * member's own Philox.  info4xk: [k][4] in fql_read_info_n's layout (device or host; host = synchronous) or NULL.  Stream and ordering
 * as fql_group_update_from_dataset. */
int fql_cfgrl_group_update_from_dataset(fql_group g, const int64_t* idx, int batch_size, const uint8_t* do_cfg, float* info4xk,
                                        void* stream);
/* fql_cfgrl_sample_actions_cfgs of every member in one fused call.  observations [k][n][od], goals [k][n][goal_dim] (NULL:
 * FQL_E_INVALID), noises [k][n][act] or NULL (then seeds [k], each member's Philox), cfgs [k][n] (one guidance weight per member and
 * row: a scalar cfg or one per member is that value repeated; host: every weight finite, else FQL_E_INVALID; or device), out
 * [k][n][act]; host or device each.  Per chunk of <= 2048 observations per member: one assemble launch (both halves; the unconditional
 * half reads each member's own unc_embed leaf), the members' sweep program over concatenated task tables and [k] argument structs, one
 * extract launch - the launch count of fql_sample_cfgs_stats, whatever k is.  out[i] is bitwise
 * fql_cfgrl_sample_actions_cfgs(member i, ..., seeds[i], cfgs[i], ...), whose row j is fql_cfgrl_sample_actions at cfg = cfgs[i][j].
 * Pointer kinds and ordering as fql_group_sample_actions. */
int fql_cfgrl_group_sample_actions(fql_group g, const float* observations, const float* goals, int n, const float* noises,
                                   const uint64_t* seeds, const float* cfgs, float* out, void* stream);
/* Launches of the group's fused update program and of one fused sampling call on a single chunk, counted from the built programs.
 * Either pointer may be NULL. */
int fql_cfgrl_group_stats(fql_group g, int64_t* launches_update, int64_t* launches_sample);

/* ---- SAC agent groups: the seeds of one RLPD run, or a target-entropy x seed sweep, advanced by one fused program (agent groups, above) ----
 * fql_sac_group_create: `members` [k], k >= 1, SAC handles (another kind: FQL_E_STATE naming it), distinct, in no group, the same batch
 * size and the same fql_config / fql_sac_config except target_entropy and target_entropy_multiplier (and the create seed); anything
 * else - tanh_squash, backup_entropy, q_agg, discount, a hidden size, a LayerNorm flag, lr - is FQL_E_INVALID naming the member and
 * target_entropy, *out NULL.  The group holds ONE fused program, one graph with a member's three lanes: the zip of every member's update
 * (blockIdx.y = member in SAC's own six kernels, concatenated task tables in the layers), a member's launch count whatever k is.  Each
 * member's target_entropy and modules_alpha/log_value stay in its own argument structs.  A member's numbers are bitwise those it has
 * alone, and after a group update it behaves as after its own: fql_read_info_n (its own 14 infos), its own updates and sampling calls,
 * fql_sac_total_loss, parameter access and checkpoints.
 * Online use: a member's replay ring is its own.  While grouped, fql_replay_create, fql_replay_add, fql_replay_size, fql_dataset_add,
 * fql_sac_sample_actions and fql_sac_total_loss on a member keep working and wait for the group's last call, as every member entry
 * point does; no group call inserts into a ring.  fql_group_destroy and fql_group_synchronize serve these groups too;
 * fql_set_batch_size and fql_destroy on a member return FQL_E_STATE while it is grouped.  fql_group_create and the other kinds' group
 * creates keep refusing SAC handles (FQL_E_STATE).  Errors: fql_last_error(NULL).
 * Across kinds: every other kind's call that takes a group returns FQL_E_STATE on a SAC group, and the four calls below that take a
 * group return it on a group of another kind, each naming the call that serves the group; a NULL group is FQL_E_INVALID. */
int fql_sac_group_create(const fql_handle* members, int k, fql_group* out);
/* fql_sac_update_from_dataset of every member in one fused update.  idx: [k][B] int64, host or device, or NULL = each member's device
 * RNG; eps_n and eps_c are each member's Philox.  info14xk: [k][14] in fql_sac_update's order (device or host; host = synchronous) or
 * NULL.  Stream and ordering as fql_group_update_from_dataset. */
int fql_sac_group_update_from_dataset(fql_group g, const int64_t* idx, int batch_size, float* info14xk, void* stream);
/* fql_sac_update_balanced of every member in one fused update (RLPD's step for k seeds): member i draws B / 2 rows of ITS OWN dataset
 * and B / 2 of ITS OWN replay ring.  idx_dataset, idx_replay: [k][B / 2] int64 each, both or neither (NULL = each member's device RNG
 * over its dataset's and its ring's current sizes), host or device; they are staged into each member's index buffer as
 * fql_sac_update_balanced stages them.  Every member is checked before any member's source is written or the graph is launched: B even,
 * a dataset uploaded, a ring created, the ring not empty - else FQL_E_INVALID naming the member, and no member's parameters, Adam
 * counts or RNG step have moved.  info14xk, stream and ordering as above. */
int fql_sac_group_update_balanced(fql_group g, const int64_t* idx_dataset, const int64_t* idx_replay, int batch_size,
                                  float* info14xk, void* stream);
/* fql_sac_sample_actions of every member in one fused call.  observations [k][n][od], noises [k][n][act] raw N(0, 1) or NULL (then seeds
 * [k], each member's Philox keyed by its own seed and the row's number in the call), one temperature for the call, out [k][n][act]; host
 * or device each.  Per chunk of <= 4096 rows per member: one assemble launch, the members' actor over concatenated task tables (its last
 * layer the [H, 2 act] head layer), one launch of SAC's action kernel, which writes the actions - 2 launches more than the actor has
 * layers, whatever k is.  out[i] is bitwise fql_sac_sample_actions(member i, ..., seeds[i], temperature, ...).  Pointer kinds and
 * ordering as fql_group_sample_actions. */
int fql_sac_group_sample_actions(fql_group g, const float* observations, int n, const float* noises, const uint64_t* seeds,
                                 float temperature, float* out, void* stream);
/* Launches of the group's fused update program and of one fused sampling call on a single chunk, counted from the built programs.
 * Either pointer may be NULL. */
int fql_sac_group_stats(fql_group g, int64_t* launches_update, int64_t* launches_sample);

#ifdef __cplusplus
}
#endif
#endif /* FQL_AMD_H */
