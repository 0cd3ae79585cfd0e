/*
 * drp.h -- C ABI of the MI355X-native particle-GNN rollout + sampling-MPC engine.
 *
 * The reference (WangYixuan12/dyn-res-pile-manip) has no FFI for this path: its
 * boundary is a Python call surface.  This header is the
 * C-ABI a Python/ctypes (or any other) host binds to get the same operations;
 * every entry point cites the reference function it replaces (paths relative to
 * the reference repo).  Plain pointers and sizes only; all float data is fp32
 * row-major; host buffers are caller-owned; device workspaces are owned by the
 * context and re-used while the shapes fit.
 *
 * Conventions
 *   - every function returns 0 on success, a negative DRP_E* code otherwise, and
 *     never throws; drp_last_error() gives the message of the last failure.
 *   - one context per GPU, one HIP stream per context.  Functions taking host
 *     buffers synchronise before returning; the drp_mpc_* family only enqueues
 *     work on the context's stream (drp_sync() waits).
 *   - B = n_sample * n_batch rows; row = sample * n_batch + batch
 *     (planners.py:336-339).  K = 10 in-edges per receiver at most
 *     (model/gnn_dyn.py:231).  F = 64 features (nf_effect).
 */
#ifndef DRP_H
#define DRP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRP_K 10
#define DRP_F 64
#define DRP_N_WEIGHTS 38403   /* floats in the state_dict, SURVEY.md 8 a16 */

enum {
    DRP_OK = 0,
    DRP_EINVAL = -1,    /* bad argument / shape */
    DRP_ESTATE = -2,    /* call order: weights / camera / goal / state not set */
    DRP_EHIP = -3,      /* HIP runtime error */
    DRP_ENOMEM = -4,
    DRP_ECOMM = -5,     /* RCCL error */
    DRP_ERANGE = -6     /* weights or inputs outside the range the split-fp16 relation encoder of
                           DRP_ENGINE_FUSED / _LITE / _SPLIT is scaled for (its hidden activations travel as two fp16
                           pieces times an exact power of two chosen from the weights): nothing was computed;
                           DRP_ENGINE_MFMA / _VALU have no such limit */
};

/* which kernels compute the MLPs */
enum {
    DRP_ENGINE_VALU = 0,  /* fp32 VALU reference kernels */
    DRP_ENGINE_MFMA = 1,  /* fp32 MFMA (v_mfma_f32_32x32x2_f32) kernels */
    DRP_ENGINE_SPLIT = 2, /* as MFMA, relation encoder on split-fp16 (two terms, 3 MFMAs per product) MFMA, fp32 accumulate */
    DRP_ENGINE_FUSED = 3, /* as SPLIT, encoder recomputed inside each aggregate: the edge-constant
                             buffer is never materialised */
    DRP_ENGINE_LITE = 4   /* opt-in: the fused engine's kernels with fewer product terms (see below); never chosen for the caller */
};
/* DRP_ENGINE_LITE -- reduced-precision forward arithmetic, selected explicitly (drp_set_engine) and by nothing else.
 *   Relation-encoder chain: ONE product per k-step, W_hi x_hi, where DRP_ENGINE_FUSED forms W_lo x_hi + W_hi x_lo + W_hi x_hi.
 *     The operands are the ones the fused engine already forms: weights rounded to nearest-even fp16 (relative 2^-11),
 *     activations rounded toward zero to fp16 (v_cvt_pkrtz_f16_f32, relative 2^-10; absolute 2^-24 in the shifted scale below
 *     fp16's normal range), the same power-of-two range shift, fp32 accumulation.  26 MFMAs per slot iteration instead of 78.
 *   Node layers (particle encoder, W_agg, the W_r | W_s projections, predictor layer 0): the two-term bf16 split with the three
 *     products w0 p0, w0 p1, w1 p0 (dropped terms <= 2^-16 relative); the third terms are neither read from LDS nor formed.
 *     72 / 48 MFMAs per tile instead of 144 / 96, 102 per encoder tile instead of 204.
 *   Everything else is the fused engine's, bit for bit: neighbour lists, gen_s_delta, reward, MPPI, the self-edge constant (full
 *     precision), the edge-chain cache, the dispatch (the same plans; the variant names carry `lite`), and the range check:
 *     DRP_ERANGE applies exactly as to DRP_ENGINE_FUSED.
 *   Forward only (drp_step, drp_forward, drp_rollout, drp_mpc_*).  With it selected, drp_gd_* and drp_train_step write their
 *     tape exactly as with DRP_ENGINE_FUSED selected (the full products; the fp32 matrix engine where the range refuses):
 *     gradients and trained weights do not depend on the choice.
 *   What it costs on given weights is what drp_accuracy_probe(engine = DRP_ENGINE_LITE) measures. */

typedef struct drp_ctx drp_ctx;

/* ---- life cycle ------------------------------------------------------------------ */
int drp_create(int device, drp_ctx** out);
void drp_destroy(drp_ctx* ctx);
const char* drp_last_error(const drp_ctx* ctx);     /* ctx may be NULL: last create error */
int drp_sync(drp_ctx* ctx);
int drp_set_engine(drp_ctx* ctx, int engine);
int drp_device_info(drp_ctx* ctx, char* name, size_t name_len, int* n_cu, size_t* hbm_bytes);

/* ---- model constants ----------------------------------------------------------- */
/* PropNetDiffDenModel.load_state_dict (visualize_mpc.py:36-41): the 38 403 floats of
 * the state_dict, concatenated in its own key order, torch Linear
 * layout [out,in].  adj_thresh = config train.particle.adj_thresh
 * (model/gnn_dyn.py:206), as the double the config holds: the radius test compares
 * against (float)(adj_thresh * adj_thresh), the product taken in doubles as Python takes
 * it (model/gnn_dyn.py:229) -- squaring the radius's fp32 rounding instead moves the
 * threshold by an ulp at 0.05, 0.1 and 0.7. */
int drp_load_weights(drp_ctx* ctx, const float* blob, size_t n_floats, double adj_thresh);

/* PlannerGD.world2cam (planners.py:192-209): m34 = first three rows of
 * inv(inv(cam_extrinsic) diag(1,-1,-1,1)) in fp32, global_scale from the config;
 * intr = env.get_cam_params() = [fx,fy,cx,cy] (env/flex_env.py:1135-1142). */
int drp_set_camera(drp_ctx* ctx, const float m34[12], float global_scale, const float intr[4]);

/* config_reward_ptcl's constants (env/flex_rewards.py:172-177, planners.py:620-624):
 * field = goal - distanceTransform(goal < 0.5), shifted to min 0, [h,w];
 * goal_coor [m,2] = (col,row) goal pixels. */
int drp_set_goal(drp_ctx* ctx, const float* field, int h, int w, const float* goal_coor, int m);

/* ---- goal pre-processing on the device (row f3) ------------------------------------------------
 * cv2.distanceTransform(src, cv2.DIST_L2, 5) (env/flex_rewards.py:174; utils.py:553,572,603):
 * distance of every non-zero pixel of src [h,w] to the nearest zero pixel.
 * DRP_DT_CV5: OpenCV's 5x5 fixed-point chamfer (weights 1, 1.4, 2.1969), same integers as its
 * two raster passes.  DRP_DT_EXACT: exact Euclidean distance (sqrt of the integer squared
 * distance, in float64, rounded to float32). */
#define DRP_DT_CV5 0
#define DRP_DT_EXACT 1
int drp_distance_transform(drp_ctx* ctx, const uint8_t* src, int h, int w, int mode, float* dist_out);

/* Everything config_reward_ptcl and the planner derive from the goal image, in one call and
 * kept on the device (replaces drp_set_goal + host work): obs_goal [h,w] = the goal distance
 * image the caller passes to trajectory_optimization_ptcl_multi_traj (planners.py:567).
 *   field     = obs_goal - distanceTransform(obs_goal < 0.5); field -= min   (env/flex_rewards.py:172-177)
 *   goal_coor = fps_np(flip((obs_goal < 0.5).nonzero()), min(max_goal_pts, count), fps_init)
 *               (planners.py:620-624; max_goal_pts = 5 * particle_num there)
 * field_out [h,w] / goal_coor_out [m,2] / m_out are optional copies for the caller. */
int drp_set_goal_image(drp_ctx* ctx, const float* obs_goal, int h, int w, int mode, int max_goal_pts,
                       int fps_init, float* field_out, float* goal_coor_out, int* m_out);

/* ---- the goal table of multi-scene sessions ----------------------------------------------------
 * A context can hold, beside its single goal, S goals of one image size (1 <= S <= DRP_MAX_SCENES): the constants of
 * config_reward_ptcl (env/flex_rewards.py:156-214) once per scene.  fields [S][h][w]; goal_coor [S][m_max][2] = (col,row)
 * with per-scene counts m [S], 1 <= m[s] <= m_max: what lies behind a scene's m[s] pixels is never read.  The table serves
 * drp_reward_scenes, drp_mpc_begin_scenes and drp_gd_begin_scenes; the single goal of drp_set_goal / drp_set_goal_image is
 * another thing: installing either leaves the other as it was.  Installing a table ends a running multi-scene session (its
 * next call returns DRP_ESTATE; begin again).  DRP_EINVAL for S outside the range or a count outside 1..m_max: the context
 * is then as it was.
 * The float64 yardsticks, training and the rewards of the one-shot rollout read the single goal only. */
#define DRP_MAX_SCENES 64
int drp_set_goal_scenes(drp_ctx* ctx, int S, const float* fields, int h, int w, const float* goal_coor, const int32_t* m,
                        int m_max);
/* The S-scene form of the goal-image call above: obs_goals [S][h][w]; slot s of the table receives the bits that call
 * produces for obs_goals[s] (the same device path, once per scene), m_max = max_goal_pts.  field_out [S][h][w] /
 * goal_coor_out [S][max_goal_pts][2] (the first m_out[s] rows of slot s) / m_out [S] are optional copies.  An image that the
 * single-scene call refuses is refused here, with its scene named, and the installed table stays. */
int drp_set_goal_image_scenes(drp_ctx* ctx, int S, const float* obs_goals, int h, int w, int mode, int max_goal_pts,
                              int fps_init, float* field_out, float* goal_coor_out, int32_t* m_out);

/* ---- single operations on host buffers (unit parity with the reference) --------
 * These stage their inputs in the buffers the drp_mpc_* / drp_gd_* sessions keep their state in: calling one of
 * them ends a running session (its next call returns DRP_ESTATE; begin again). */
/* PlannerGD.gen_s_delta (planners.py:211-257). s_cur [B,N,3], action [B,4] -> [B,N,3] */
int drp_gen_s_delta(drp_ctx* ctx, const float* s_cur, const float* action, int B, int N,
                    float* s_delta_out);

/* The graph of predict_one_step (model/gnn_dyn.py:223-251) as receiver-major lists:
 * nbr_idx [B,N,10] int16 (ascending sender, -1 padded), nbr_cnt [B,N] uint8. */
int drp_build_graph(drp_ctx* ctx, const float* s_cur, const float* s_delta, int B, int N,
                    int16_t* nbr_idx_out, uint8_t* nbr_cnt_out);

/* PropNetDiffDenModel.predict_one_step (model/gnn_dyn.py:209-254).
 * a_cur [B,N], s_cur/s_delta [B,N,3], dens [B] -> s_pred [B,N,3] */
int drp_step(drp_ctx* ctx, const float* a_cur, const float* s_cur, const float* s_delta,
             const float* dens, int B, int N, float* s_pred_out);

/* PropModuleDiffDen.forward (model/gnn_dyn.py:147-198) with the relations given as
 * lists instead of dense one-hot Rr/Rs. */
int drp_forward(drp_ctx* ctx, const float* a_cur, const float* s_cur, const float* s_delta,
                const float* dens, const int16_t* nbr_idx, const uint8_t* nbr_cnt, int B, int N,
                float* s_pred_out);

/* PlannerGD.ptcl_model_rollout (planners.py:302-370): s0 [nb,N,3], attr [nb,N],
 * dens [nb], actions [B,H,4] -> states_out [B,H,N,3] (nullable).  If reward_out is
 * not NULL it receives config_reward_ptcl of every step, [B,H] (what
 * ptcl_evaluate_traj computes, planners.py:414-422); needs drp_set_goal. */
int drp_rollout(drp_ctx* ctx, const float* s0, const float* attr, const float* dens, int nb,
                int N, const float* actions, int B, int H, float* states_out, float* reward_out);

/* config_reward_ptcl (env/flex_rewards.py:156-214) downstream of the distance
 * transform.  state [Bp,N,3] -> reward [Bp]. */
int drp_reward(drp_ctx* ctx, const float* state, int Bp, int N, int normalize, float* reward_out);
/* The same with a goal per row: row r is scored against scene[r] of the goal table (env/flex_rewards.py:156-214 with that
 * scene's constants) and gets the bits the call above gives with that scene's goal installed alone.  scene [Bp] int32.
 * DRP_ESTATE without a table, DRP_EINVAL for an index outside 0..S-1.  Ends no session. */
int drp_reward_scenes(drp_ctx* ctx, const float* state, const int32_t* scene, int Bp, int N, int normalize,
                      float* reward_out);

/* ---- device-resident sampling MPC (MPPI) ------------------------------------------
 * One iteration = sample_action_sequences (planners.py:69-190) -> ptcl_model_rollout
 * -> final-step reward -> optimize_action (planners.py:549-561), all on the stream.
 * The sample axis may be sharded over ranks: each rank runs n_sample_local samples
 * and the softmax-weighted mean is combined from per-rank partials. */
typedef struct drp_mpc_params {
    int n_batch;          /* initial-state columns (particle re-samplings) */
    int n_particles;
    int n_sample;         /* samples on THIS rank */
    int n_look_ahead;     /* H */
    double sigma;         /* mpc.sigma * global_scale / 12 (planners.py:116) */
    double beta_filter;   /* mpc.mppi.beta_filter (planners.py:93) */
    double reward_weight; /* mpc.mppi.reward_weight (planners.py:553) */
    float act_lo[4];      /* clip box (planners.py:152-155) */
    float act_hi[4];
    uint64_t seed;        /* Philox key: the stream below */
    uint64_t sample_offset; /* first global sample index of this rank (Philox counter) */
    int noise_type;       /* DRP_NOISE_*: the sampler's noise_type argument (planners.py:75,116-135,169-175) */
    int reserved;         /* 0 */
} drp_mpc_params;
#define DRP_NOISE_NORMAL 0      /* N(0, sigma)                                                  */
#define DRP_NOISE_UNIFORM 1     /* U(-sigma, sigma); the caller passes sigma = 2 global_scale / 12 */
#define DRP_NOISE_TOTAL_RAND 2  /* no residual: every push drawn uniformly from the clip box   */

int drp_mpc_begin(drp_ctx* ctx, const drp_mpc_params* p, const float* s0, const float* attr,
                  const float* dens, const double* nominal /* [H,4] */);
/* drp_mpc_begin without the goal (weights and a camera only): a session on a cost of the caller's.  drp_mpc_rollout(ctx, 0) then
 * runs the rollout and no reward kernel (a non-zero reward_all_steps: DRP_EINVAL); the caller reads the states (drp_mpc_get),
 * computes a reward per row and hands them in: drp_mpc_set_rewards(rewards [rows]) writes the final-step slot the update kernels
 * read.  After a rollout and before drp_mpc_set_rewards, drp_mpc_partials, drp_mpc_update*, drp_mpc_elite and
 * drp_mpc_fetch_async return DRP_ESTATE in such a session (drp_mpc_get's rewards are then undefined).  drp_mpc_set_rewards is
 * accepted in a session begun by drp_mpc_begin too, where it replaces the rewards; NaN rewards are the update kernels' to handle
 * as they handle their own; a null pointer gives DRP_EINVAL, a multi-scene session DRP_ESTATE.  Cost sessions are single-scene. */
int drp_mpc_begin_cost(drp_ctx* ctx, const drp_mpc_params* p, const float* s0, const float* attr,
                       const float* dens, const double* nominal /* [H,4] */);
int drp_mpc_set_rewards(drp_ctx* ctx, const float* rewards /* [rows] */);
/* A session over S scenes (1 <= S <= DRP_MAX_SCENES, the S of the installed goal table): S piles, S goals, S nominal
 * sequences, planned in one rollout batch.  p is shared by all scenes (shapes, sigma, beta_filter, reward_weight, clip box,
 * noise type, sample_offset); p->n_sample is PER SCENE; p->seed is ignored for seeds [S].  s0 [S * nb][N][3], attr
 * [S * nb][N], dens [S * nb] (scene-major: scene s owns columns s * nb .. s * nb + nb - 1), nominal [S][H][4].
 * Rows follow planners.py:661-662 with S * nb columns:
 *     row = (sample * S + scene) * nb + column,   scene(row) = (row / nb) % S,   B = n_sample * S * nb
 * so the rollout is the one of a single-scene session of S * nb columns, and a row's reward reads its scene's goal.
 * Every session call then acts on all scenes: drp_mpc_sample draws scene s from nominal[s] with the Philox key seeds[s] and
 * a single-scene session's counter (the same draws; host noise is [S][n_sample][H][4]); drp_mpc_set_actions, drp_mpc_get,
 * drp_mpc_fetch_async / drp_mpc_wait move B rows and [S][H][4] nominals; drp_mpc_update_device and
 * drp_mpc_update_elite_device run one softmax combine / elite selection per scene over that scene's samples, in a
 * single-scene session's reduction order: scene s's nominal and statistics are the doubles of a single-scene session with
 * seed = seeds[s].  Sample indices are per scene, 0 .. n_sample - 1 plus sample_offset.
 * The range check (DRP_ERANGE) is taken once per session over ALL scenes' attributes and densities and the clip box: one
 * out-of-range scene refuses -- or, with the host mirror's fallback, moves to the fp32 matrix engine -- the whole session.
 * Sharded multi-scene planning is out of scope: with S > 1 the partials / update / elite / update_elite calls (the
 * host-transport forms) and the two device updates with a communicator of more than one rank return DRP_ESTATE.
 * DRP_ESTATE without a goal table; DRP_EINVAL for S out of range or a table of another S. */
int drp_mpc_begin_scenes(drp_ctx* ctx, const drp_mpc_params* p, int S, const float* s0, const float* attr,
                         const float* dens, const double* nominal /* [S][H][4] */, const uint64_t* seeds /* [S] */);
/* the statistics of the last update, per scene: [S][6] = mean r, unbiased std r, max r, argmax (sample index within the
 * scene, plus sample_offset), Z, m.  S = 1 for a single-scene session. */
int drp_mpc_stats_scenes(drp_ctx* ctx, double* stats_out /* [S][6] */);
/* noise: NULL -> device Philox draws; else host [n_sample,H,4] draws: standard normal (DRP_NOISE_NORMAL),
 * U(-1,1) (DRP_NOISE_UNIFORM) or U[0,1) (DRP_NOISE_TOTAL_RAND).
 * The device's stream is a contract (sharding rests on it: a shard of a job draws what the whole job draws), restated on
 * the host in tests/_philox_ref.py and held to it by tests/test_gpu_sampler.py:
 *   block    w[0..3] = Philox4x32-10 (Random123: multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85)
 *            key     (seed & 0xffffffff, seed >> 32)              -- a scene of a multi-scene session: seeds[scene]
 *            counter (gs & 0xffffffff, gs >> 32, t, iteration & 0xffffffff),   gs = sample_offset + sample (mod 2^64),
 *                    t = 0 .. H-1 the step: one block per (global sample, step); `iteration` enters modulo 2^32
 *   uniform  component c = 0..3 of the push reads w[c]:  u = (w[c] >> 8) * 2^-24 in [0, 1), 24 bits, exact;
 *            DRP_NOISE_UNIFORM draws 2u - 1, DRP_NOISE_TOTAL_RAND u
 *   normal   components 0, 1 read the pair (a, b) = (w[0], w[1]), components 2, 3 the pair (w[2], w[3]) (Box-Muller):
 *            u1 = ((float)a + 1) * 2^-32 in (0, 1],  u2 = (float)b * 2^-32,  r = sqrt(-2 ln u1) <= 6.66,
 *            even component r cos(2 pi u2), odd component r sin(2 pi u2) -- float32, round to nearest: the uniforms are the
 *            restatement's bits, a normal is within a few float32 ulps of r of the float64 evaluation on the same u1, u2
 *            (the bound: DESIGN.md section 2, row a12)
 *   filter   per component, in float64:  resid = beta (sigma n) + resid (1 - beta),  push = clip(nominal[t] + resid) (TOTAL_RAND:
 *            act_lo + n (act_hi - act_lo)), rounded to float32 -- the restatement's bits for device and host draws alike;
 *            every column of a sample gets the sample's push. */
int drp_mpc_sample(drp_ctx* ctx, const float* noise, uint64_t iteration);
int drp_mpc_set_actions(drp_ctx* ctx, const float* actions /* [B,H,4] */);
int drp_mpc_rollout(drp_ctx* ctx, int reward_all_steps);
/* per-rank partials of the softmax mean over column `col`'s samples:
 * out[0]=m, out[1]=Z, out[2..2+4H)=A, then sum r, sum r^2, max r, argmax (as double). */
int drp_mpc_partials(drp_ctx* ctx, double* out /* [6+4H], nullable */);
/* combine `n_ranks` partial records (as returned above, concatenated) into the new
 * nominal sequence; uploads it as the next iteration's nominal. */
int drp_mpc_update(drp_ctx* ctx, const double* partials, int n_ranks, double* nominal_out);
/* partials -> (RCCL all-gather if a communicator is attached) -> update, no host hop */
int drp_mpc_update_device(drp_ctx* ctx);
/* Elite (cross-entropy-method style) update -- NOT in the reference (planners.py has no CEM; SURVEY.md section 8e
 * lists it as the other form of the planner's one exchange): the new nominal sequence is the mean of the k best
 * samples' sequences, higher final-step reward first, ties to the lower global sample index.
 * drp_mpc_elite: this rank's k best as records [reward, global sample index, act[4H]] (2 + 4H doubles each, best
 * first; reward = -inf and index = -1 pad a rank with fewer than k samples).
 * drp_mpc_update_elite: combine n_ranks x k records (host transport) into the nominal sequence.
 * drp_mpc_update_elite_device: the rank's statistics record (as drp_mpc_update_device) and its k elite records
 * travel as ONE message, [6 + 4H | k (2 + 4H)] doubles, in ONE RCCL all-gather per iteration when a communicator is
 * attached, and both combines read the gathered messages in place; no host hop.  1 <= k <= 1024, up to 9 000
 * samples per rank. */
int drp_mpc_elite(drp_ctx* ctx, int k, double* out /* [k][2+4H], nullable */);
int drp_mpc_update_elite(drp_ctx* ctx, const double* records, int n_ranks, int k, double* nominal_out /* [H][4], nullable */);
int drp_mpc_update_elite_device(drp_ctx* ctx, int k);
int drp_mpc_get(drp_ctx* ctx, float* actions /*[B,H,4]*/, float* rewards /*[B] final*/,
                float* rewards_all /*[B,H]*/, float* states /*[B,H,N,3]*/, double* nominal);
/* The pushes and final rewards of the iteration just enqueued, without a host wait: slot (0 or 1) takes them into pinned
 * memory behind the iteration's kernels -- before the next drp_mpc_sample overwrites the pushes --; drp_mpc_wait(slot)
 * blocks until they are there and copies them out (each pointer nullable).  The planner's loop enqueues iteration i + 1
 * before it waits for iteration i.  A slot must be waited for before it is used again; drp_mpc_begin and the one-shot
 * calls drop what is in flight. */
int drp_mpc_fetch_async(drp_ctx* ctx, int slot);
int drp_mpc_wait(drp_ctx* ctx, int slot, float* actions /*[B,H,4]*/, float* rewards /*[B] final*/);

/* fps_np (utils.py:451-466): farthest-point subsample of pts [n,dim] (dim 2 or 3) to k points
 * starting from init_idx; idx_out [k] are indices into pts, max_dist_out the largest distance
 * of any point to the chosen set.  Used for the goal pixels (planners.py:620-624). */
int drp_fps(drp_ctx* ctx, const float* pts, int n, int dim, int k, int init_idx, int32_t* idx_out,
            float* max_dist_out);

/* ---- training on the same kernels (row f4; train/train_gnn_dyn.py:159-214) ---------------------
 * One iteration of the reference's training loop body for one collated batch
 * (train/train_gnn_dyn.py:20-45 collate_fn: samples zero-padded to the batch's largest
 * particle count N):
 *   s_cur = states[:, 0]; for t < n_rollout: s_pred = predict_one_step(attrs[:, 0], s_cur,
 *   states_delta[:, t], particle_dens); loss += sum_b mse(s_pred[b, :n_b], states[b, t+1, :n_b]);
 *   s_cur = s_pred;  loss /= n_rollout * B;  loss.backward();  Adam(lr, betas=(beta1, .999)).step()
 * states [B, n_rollout+1, N, 3], states_delta [B, n_rollout, N, 3], attrs [B, n_rollout+1, N],
 * particle_nums [B], particle_dens [B].  loss_out receives the loss (before the update),
 * grad_out (nullable, 38 403 floats in state_dict order) the gradient of every parameter.
 * The arrays are copied before the call returns (one upload), and the call returns when the iteration is complete on
 * the device (its only host wait): the caller's buffers are free at once, drp_get_weights serves the updated weights. */
#define DRP_TRAIN_EVAL 0     /* loss only ('valid' phase, torch.set_grad_enabled(False)) */
#define DRP_TRAIN_GRAD 1     /* loss + gradients, weights untouched */
#define DRP_TRAIN_UPDATE 2   /* loss + gradients + one Adam step on the context's weights */
int drp_train_begin(drp_ctx* ctx, int n_rollout, double lr, double beta1);
int drp_train_step(drp_ctx* ctx, const float* states, const float* states_delta, const float* attrs,
                   const int32_t* particle_nums, const float* particle_dens, int B, int N, int mode,
                   double* loss_out, float* grad_out);
/* drp_train_step with the loss of each step taken against an UNTRACKED cloud: same arguments, then the targets.  Row i of a
 * target is not particle i of the prediction (a pile re-sampled by FPS after every push, env/flex_env.py:1020,1093; a depth
 * camera's cloud), so the term of (step t, sample b) is the symmetric squared Chamfer distance of drp_cloud_chamfer below between
 * s_pred_t[b, :n_b] and targets[b, t, :target_nums[b, t]], (fwd + bwd) / (n_rollout B), summed step-major as drp_train_step's;
 * the arg-mins are constants of the derivative.  Of states [B, n_rollout+1, N, 3] only step 0 is read (the layout is
 * drp_train_step's); the impulses are data, as there: with n_rollout = 1 and Engine.gen_s_delta on the observed cloud this is
 * exact for real untracked data, longer rollouts serve recorded episodes whose correspondence is dropped.  targets
 * [B, n_rollout, M, 3], target_nums [B, n_rollout].  Everything behind the loss gradient -- reverse pass, weight gradients, Adam,
 * re-packing -- is drp_train_step's.  DRP_ESTATE without drp_train_begin; DRP_EINVAL for a null argument, a count outside 1..N
 * or 1..M, M outside 1..4096. */
int drp_train_step_untracked(drp_ctx* ctx, const float* states, const float* states_delta, const float* attrs,
                             const int32_t* particle_nums, const float* particle_dens, int B, int N,
                             const float* targets /*[B][H][M][3]*/, const int32_t* target_nums /*[B][H]*/, int M,
                             int mode, double* loss_out, float* grad_out);
/* drp_train_step (targets == NULL, M == 0: the tracked MSE) or drp_train_step_untracked (otherwise: the Chamfer loss) with every
 * step's impulse computed from the batch's pushes ON THE STATE THE STEP READS, as every consumer of the trained model does:
 * train/train_gnn_dyn.py:159-189 with states_delta[:, t] replaced by planners.py:211-257 evaluated at s_cur.  actions
 * [B, n_rollout, 4] = (sx, sy, ex, ey) in world units, the planner's convention, through the camera of drp_set_camera.
 *   forward   s_cur_0 = states[:, 0], s_cur_t = s_pred_{t-1}; row n < particle_nums[b] of step t's impulse is
 *             gen_s_delta(s_cur_t[b], actions[b, t])[n] with the arithmetic (and on those rows the bits) of drp_gen_s_delta; rows
 *             n >= particle_nums[b] get +0.0f, what collate_fn's padding carries as data -- they still join the graph.
 *   backward  for t > 0 and real rows d loss / d s_pred_{t-1}[b, n] += J_pos^T g_s_delta_t[b, n]: the hard mask 0 < u < L is a
 *             constant of the derivative, the soft mask and both projections are differentiated (as drp_gd_grad); padded rows
 *             receive nothing.  Per element the order is fixed -- loss seed, residual share, relation-encoder share, push share
 *             -- and nothing is atomic: two runs give the same bits.  d loss / d actions is no output: the pushes are data.
 * Loss, weight gradients, Adam, re-packing and the one wait are drp_train_step's; with n_rollout = 1 the result has the bits of
 * drp_train_step fed drp_gen_s_delta's impulses with the padded rows zeroed.  The tape engine's range check takes the pushes'
 * length bound where drp_train_step takes max |states_delta|.  DRP_ESTATE without drp_train_begin or without a camera;
 * DRP_EINVAL for a null argument (actions included), a push of zero length in the camera frame (0 / 0 in every impulse, and
 * from there in every weight; the dataset path refuses such a push too), and whatever drp_train_step(_untracked) refuses.  A
 * refused call leaves the context as it was. */
int drp_train_step_actions(drp_ctx* ctx, const float* states, const float* actions /*[B][H][4]*/, const float* attrs,
                           const int32_t* particle_nums, const float* particle_dens, int B, int N,
                           const float* targets /*[B][H][M][3] or NULL*/, const int32_t* target_nums /*[B][H] or NULL*/, int M,
                           int mode, double* loss_out, float* grad_out);
int drp_train_set_lr(drp_ctx* ctx, double lr);
/* model.state_dict() (train/train_gnn_dyn.py:226,244): the current weights, drp_load_weights layout */
int drp_get_weights(drp_ctx* ctx, float* blob_out, size_t n_floats);

/* ---- particle extraction from the depth image (row f2; env/flex_env.py:933-951) --------------
 * The reference runs this chain on the host between every pair of planner calls, 30 times per
 * observation (batch_size=30, env/flex_env.py:1020,1093).  All clouds are float64 [n,3] in the
 * camera frame, exactly as the reference's numpy arrays. */

/* utils.py:491-506 depth2fgpcd(depth, mask, cam_params): row-major foreground pixels
 * (mask != 0 and depth > 0) -> points ((x-cx)*d/fx, (y-cy)*d/fy, d).  mask NULL selects the
 * rule of env/flex_env.py:945, depth < 0.599/0.8 in float32.  cam = {fx, fy, cx, cy}.
 * pcd_out may be NULL (count only); DRP_EINVAL if cap < n (n_out is still set). */
int drp_depth2fgpcd(drp_ctx* ctx, const float* depth, const uint8_t* mask, int h, int w, const double cam[4],
                    double* pcd_out, int cap, int* n_out);

/* utils.py:533-544 downsample_pcd(pcd, voxel_size) = open3d voxel_down_sample: one point per
 * occupied voxel (index floor((p - (min_bound - voxel/2)) / voxel)), the mean of its points
 * summed in index order; voxels are emitted in ascending (ix, iy, iz) (open3d's order is that
 * of an unordered_map, i.e. unspecified). */
int drp_downsample_pcd(drp_ctx* ctx, const double* pcd, int n, double voxel, double* out, int cap, int* m_out);

/* utils.py:423-436 fps(pcd, particle_num, init_idx) for `batch` independent starts:
 * dgl.geometry.farthest_point_sampler on the float32 copy of the cloud (squared float32
 * distances, first maximum), pts_out[batch, npoints, 3] float32 = the chosen points,
 * r_out[batch] = max_i min_j |pcd_i - pts_j| in float64.  init_idx NULL: start b is drawn
 * from `seed` (dgl draws it from torch's global generator). */
int drp_fps_pcd(drp_ctx* ctx, const double* pcd, int n, int npoints, int batch, const int32_t* init_idx,
                uint64_t seed, float* pts_out, double* r_out);

/* utils.py:438-449 fps_rad(pcd, radius): farthest-point sampling of the float64 cloud from
 * `init_idx` (the reference draws it from numpy's global generator) until every point is within
 * `radius` of a sample -- the dataset's sampler (dataset/dataset_gnn_dyn.py:99).  idx_out holds
 * up to `cap` indices into pcd, count_out how many were chosen (cap reached: sampling stops). */
int drp_fps_rad(drp_ctx* ctx, const double* pcd, int n, double radius, int init_idx, int cap, int32_t* idx_out,
                int* count_out);

/* utils.py:468-477 recenter(pcd, sampled_pcd, r): out[b, j] = float32 mean of the cloud points
 * with |p - sampled[b, j]| < r[b] (NaN when there is none, as numpy's mean of an empty set). */
int drp_recenter(drp_ctx* ctx, const double* pcd, int n, const float* sampled, int npoints, int batch,
                 const double* r, float* out);

/* env/flex_env.py:933-951 FlexEnv.obs2ptcl_fixed_num_batch(obs, particle_num, batch_size), the
 * whole chain on the device with one upload and one download: depth_raw = obs[..., -1] [h, w]
 * (world units), depth = depth_raw / global_scale, foreground depth < 0.599/0.8, voxel 0.01,
 * recentering radius min(0.02, 0.5 * particle_r).  ptcl_out[batch, npoints, 3] float64 (float32
 * values, as the reference's array), r_out[batch] = particle_r (dens = 1 / r^2,
 * env/flex_env.py:1022).  n_fg / n_down (nullable) return the cloud sizes. */
int drp_obs2ptcl(drp_ctx* ctx, const float* depth_raw, int h, int w, float global_scale, const double cam[4],
                 int npoints, int batch, const int32_t* init_idx, uint64_t seed, double* ptcl_out, double* r_out,
                 int* n_fg, int* n_down);

/* ---- gradient-descent planner (the reference's live mpc_type 'GD') ----------------------------
 * One iteration of planners.py:682-764: rollout -> final-step reward -> loss = -sum(reward)
 * -> d loss / d pushes by reverse mode (through every step of the horizon) -> Adam(lr) step
 * -> clip box.  actions [B,H,4] with B = traj_num * n_batch rows (row = traj * n_batch + batch).
 * The forward pass writes its tape on the fused engine (also when DRP_ENGINE_LITE is selected: the tape never uses the reduced
 * products); when drp_set_engine has selected an fp32 engine, or the weights /
 * inputs are outside the split-fp16 relation encoder's range, on the fp32 matrix engine instead (slower, same gradients
 * to fp32 rounding): drp_gd_* and drp_train_step never return DRP_ERANGE -- env/flex_env.py:973-976 accepts no other
 * planner than this one. */
int drp_gd_begin(drp_ctx* ctx, const float* s0, const float* attr, const float* dens, int nb, int N,
                 const float* actions, int B, int H, double lr, const float act_lo[4], const float act_hi[4]);
/* forward + backward only: rewards [B], d loss / d actions [B,H,4], d loss / d state_pred
 * [B,H,N,3] (each nullable).  The reward's gradient follows the reference's own operations where they are not smooth
 * (drp_gd_grad_f64 too): grid_sample's border clamp passes no gradient where ix <= 0 or ix >= W - 1, the border itself
 * included; a goal pixel equidistant from several particles belongs to the one of the lowest index; and a goal pixel that IS
 * its nearest particle's pixel (distance 0) contributes nothing to the gradient -- torch.norm's backward at 0, never 0 / 0.
 * The rewards are drp_reward's bits. */
int drp_gd_grad(drp_ctx* ctx, float* rewards_out, float* grad_act_out, float* grad_state_out);
/* one full iteration (forward, backward, Adam, clip); rewards of the iterate BEFORE the update */
int drp_gd_step(drp_ctx* ctx, float* rewards_out);
int drp_gd_get(drp_ctx* ctx, float* actions_out);
/* The same iteration without a host wait: slot (0 .. DRP_GD_SLOTS - 1) takes the iteration's rewards (of the iterate
 * before the update) and the updated pushes in pinned memory, written by the iteration's own kernels (no copy on the
 * stream); drp_gd_wait(slot) blocks until they are there and copies them out (each pointer nullable).  The planner's loop
 * keeps a few iterations enqueued ahead of the one it waits for, so the per-iteration bookkeeping of planners.py:721-738
 * runs beside the device instead of between its iterations.
 * A slot must be waited for before it is used again; drp_gd_begin and the one-shot calls drop what is in flight. */
#define DRP_GD_SLOTS 8
int drp_gd_step_async(drp_ctx* ctx, int slot);
int drp_gd_wait(drp_ctx* ctx, int slot, float* rewards_out, float* actions_out);
/* The same session over S scenes (the S of the installed goal table): s0 [S * nb][N][3], attr [S * nb][N], dens [S * nb],
 * scene-major; B a multiple of S * nb; row r belongs to scene (r / nb) % S (planners.py:661-662 with S * nb columns) and its
 * reward and the reward's gradient read that scene's goal (env/flex_rewards.py:156-214).  Rows are independent Adam problems,
 * so nothing is combined per scene: the five session calls above then run as they do in a single-scene session, on either
 * tape, and a row's rewards, gradients and pushes are the bits of a single-scene session on its scene.  The tape's engine
 * is picked once from all scenes' attributes, densities and pushes.  DRP_ESTATE without a goal table; DRP_EINVAL for S out
 * of range, a table of another S, or B no multiple of S * nb.  Sharding the rows of a multi-scene session over ranks is out
 * of scope, as for the sampling sessions. */
int drp_gd_begin_scenes(drp_ctx* ctx, int S, const float* s0, const float* attr, const float* dens, int nb, int N,
                        const float* actions, int B, int H, double lr, const float act_lo[4], const float act_hi[4]);

/* ---- planning on a caller's cost: predicted states out, state-gradient seed in ----------------------------------------------
 * The planner's counterpart of drp_train_predict / drp_train_step_seeded: the loss is the caller's, everything behind its state
 * gradient is the session's own code (forward with tape, reverse mode through every step, Adam, clip).
 * drp_gd_begin_cost: drp_gd_begin without the goal -- weights and a camera only; the same engine pick, buffers and Adam reset.
 * In such a session drp_gd_grad, drp_gd_step, drp_gd_step_async and drp_gd_wait return DRP_ESTATE (the message names the
 * seeded calls); drp_gd_get works.  The three calls below also work in a session begun by drp_gd_begin (the goal is not read);
 * after drp_gd_begin_scenes they return DRP_ESTATE.
 * drp_gd_predict: the forward with tape on the session's current pushes EXACTLY as drp_gd_grad runs it (the same tape engine, the
 * same self-edge constants), no reward: states_out [B][H][N][3], every step's predicted state.  No push, Adam moment or
 * iteration count changes.
 * drp_gd_grad_seeded: the forward again (deterministic: the bits drp_gd_predict returned), then the reverse pass with seed
 * [B][H][N][3], seed[b, t, n, :] = d loss / d s_pred_t[b, n], COMPLETE: nothing is scaled, the sign is the caller's, the library
 * minimises.  Step H-1's seed is d loss / d state_{H-1} as the built-in reward's gradient is; the seed of a step t < H-1 joins
 * d loss / d state_t at ONE point of its sum, in fp32 and in float64 alike: residual share of step t+1's gradient, THEN THE SEED,
 * then the relation encoder's share (own slots, then the reversed lists), then gen_s_delta's position share.  grad_act_out
 * [B][H][4], grad_state_out [B][H][N][3] = the total d loss / d state_t, seed included (each nullable).  With seed = 0 but
 * seed[:, H-1] = drp_gd_grad's grad_state[:, H-1], both outputs equal drp_gd_grad's as numbers (x + 0.0 may turn -0.0 into +0.0).
 * drp_gd_step_seeded: the same plus the Adam step and the clip of drp_gd_step -- the update rides on the last kb_sdelta launch,
 * the same arithmetic --, the iteration count advances, one wait; actions_out [B][H][4] (nullable): the updated pushes.
 * The seed goes up in one copy and is re-laid step-major on the device.  DRP_ESTATE outside a GD session or in a multi-scene one;
 * DRP_EINVAL for a null seed / states_out, or a seed value that is infinite or not a number (the message names row, step and
 * particle).  A refused call leaves pushes, moments and iteration count as they were.  Stateless on purpose: drp_gd_predict's
 * tape is not kept for the following step (that would need a validity mark over every call that touches the workspace); the
 * price is one forward per iteration. */
int drp_gd_begin_cost(drp_ctx* ctx, const float* s0, const float* attr, const float* dens, int nb, int N,
                      const float* actions, int B, int H, double lr, const float act_lo[4], const float act_hi[4]);
int drp_gd_predict(drp_ctx* ctx, float* states_out /*[B][H][N][3]*/);
int drp_gd_grad_seeded(drp_ctx* ctx, const float* seed /*[B][H][N][3]*/, float* grad_act_out, float* grad_state_out);
int drp_gd_step_seeded(drp_ctx* ctx, const float* seed /*[B][H][N][3]*/, float* actions_out /*[B][H][4], nullable*/);

/* ---- planning to a target cloud on the device ----------------------------------------------------------------------------------
 * The goal as a cloud: how much material belongs where, in the camera frame the predicted states live in.  One target cloud is
 * installed on the context BESIDE the image goal and the goal table (it touches neither); a cloud session is drp_mpc_begin /
 * drp_gd_begin with that cloud in the image's place, and no state, reward or seed crosses the bus inside an iteration.
 *   value(row) = chamfer: fwd + bwd of drp_cloud_chamfer(final state of the row, target)            (their bits)
 *                sinkhorn: drp_cloud_divergence(final state, target) with eps = eps_scale / dens[row % n_batch], `iters` sweeps
 *                          and scale 1 (its bits; the target's own self problem is solved once per start column at the begin)
 *   reward(row) = (float)(-((double)weight * value));   gradient = weight x d value / d state_{H-1}: the one-shot's double
 *                 expression times the weight, rounded to fp32 ONCE (a weight that is a power of two gives weight x the
 *                 one-shot's fp32 gradient exactly).
 * drp_set_goal_cloud: q [M][3], M <= 4096 (chamfer) or 1024 (sinkhorn); weight > 0 and finite; eps_scale > 0 and iters in
 * 1..DRP_TRANSPORT_MAX_ITERS are read for the sinkhorn kind only.  DRP_EINVAL for a null or non-finite q, M out of range, a bad
 * kind or parameter.  Installing a goal ends a running CLOUD session (its tables were the old goal's); other sessions go on.
 * drp_mpc_begin_cloud: drp_mpc_begin's arguments; needs weights, a camera and a cloud goal (DRP_ESTATE without), N within the
 * kind's limit and for sinkhorn positive finite densities (DRP_EINVAL).  drp_mpc_rollout(ctx, 0) then runs the rollout and the
 * cloud reward kernel on every row's final state, writing the slot the update kernels read (a non-zero reward_all_steps:
 * DRP_EINVAL).  Every later session call works as after drp_mpc_begin; drp_mpc_set_rewards stays accepted and replaces the rewards.
 * drp_gd_begin_cloud: drp_gd_begin's arguments; drp_gd_grad, drp_gd_step, drp_gd_step_async, drp_gd_wait and drp_gd_get work as
 * in a goal session: the cloud kernel stands where the image reward's launch stood, writes the rewards (and their pinned copy) and
 * d loss / d state_{H-1}; no seed is staged and the forward runs once per iteration.  The seeded calls work as after drp_gd_begin.
 * drp_cloud_goal_eval: the installed goal on the caller's clouds p [B][N][3] with n_p [B] real rows (null: all N; counts outside
 * 1..N: DRP_EINVAL) and for sinkhorn dens [B] (eps = eps_scale / dens[b]; ignored, nullable, for chamfer): rewards_out [B],
 * values_out [B] = weight x value as a double, grad_out [B][N][3] (padded rows +0.0), each nullable.  A one-shot: it needs no
 * weights and ends no session.  A non-finite coordinate is not refused: that row's reward is NaN after the same number of
 * steps, every other row's outputs keep their bits.
 * Cloud sessions are single-scene and balanced: a goal cloud per scene and a reach (unbalanced masses) are out of scope.
 * Cost, measured on one MI355X (profiles/cloud_goal_timing.txt; target as large as the pile): a chamfer session runs at the
 * image goal's speed (0.59 / 2.79 / 8.86 ms per MPPI iteration at 1 024 samples x 20 / 100 / 300 particles x H 10 against 0.59 /
 * 2.81 / 9.12 ms; 0.79 / 3.39 ms per GD iteration at 1 500 rows x 20 / 100 x H 3 against 0.78 / 3.38 ms).  A sinkhorn goal at
 * iters 50 is K N M double exponentials per row and costs MORE than the rollout: 1.83 / 8.16 / 40.1 ms and 2.55 / 11.4 ms, 2.9 -
 * 4.4 image-goal iterations; linear in iters.  Both are faster than the same cost through drp_mpc_set_rewards /
 * drp_gd_step_seeded (1.2 - 1.8 x and 1.3 - 1.5 x). */
#define DRP_CLOUD_CHAMFER 0
#define DRP_CLOUD_SINKHORN 1
typedef struct drp_cloud_goal_params {
    int kind;                   /* DRP_CLOUD_CHAMFER, DRP_CLOUD_SINKHORN */
    int iters;                  /* sinkhorn: sweeps, 1..DRP_TRANSPORT_MAX_ITERS */
    double weight;              /* > 0, finite */
    double eps_scale;           /* sinkhorn: > 0, finite */
} drp_cloud_goal_params;
int drp_set_goal_cloud(drp_ctx* ctx, const float* q /*[M][3]*/, int M, const drp_cloud_goal_params* p);
int drp_mpc_begin_cloud(drp_ctx* ctx, const drp_mpc_params* p, const float* s0, const float* attr,
                        const float* dens, const double* nominal /* [H,4] */);
int drp_gd_begin_cloud(drp_ctx* ctx, const float* s0, const float* attr, const float* dens, int nb, int N,
                       const float* actions, int B, int H, double lr, const float act_lo[4], const float act_hi[4]);
int drp_cloud_goal_eval(drp_ctx* ctx, const float* p /*[B][N][3]*/, const int32_t* n_p /*[B], nullable*/,
                        const float* dens /*[B], sinkhorn only*/, int B, int N, float* rewards_out /*[B]*/,
                        double* values_out /*[B]*/, float* grad_out /*[B][N][3]*/);

/* ---- multi-GPU (RCCL over xGMI) ------------------------------------------------------
 * The library does not link librccl: the first of these calls binds, at run time, $DRP_RCCL_LIB, else the librccl that
 * sits NEXT TO THE HIP RUNTIME THIS LIBRARY RUNS ON (PyTorch's bundled pair when the host imported torch first, /opt/rocm's
 * when torch came later or not at all: a wheel imported afterwards brings a second HIP runtime into the process, and its
 * RCCL would talk to that one), else a librccl the process has already mapped, else /opt/rocm's.  drp_comm_info reports
 * which one.
 * Hang guard: while a communicator is attached, every host wait of the context (drp_sync, drp_mpc_wait, drp_gd_wait,
 * the waits inside the blocking calls) polls the stream, the communicator's asynchronous error and a deadline
 * (env DRP_COMM_TIMEOUT_S, default 60; DRP_COMM_INIT_TIMEOUT_S, default 300, for drp_comm_init).  On error or
 * timeout the communicator is aborted (ncclCommAbort) and the call returns DRP_ECOMM.  The failure is STICKY: until
 * drp_comm_destroy (continue alone) or a fresh drp_comm_init, every entry point that would have combined the ranks' shards
 * (drp_mpc_update_device, drp_mpc_update_elite_device, drp_comm_allgather) returns DRP_ECOMM too -- none of them quietly
 * carries on with this rank's data.  What needs no other rank (rollouts, rewards, fetches) keeps working.  The helper
 * threads behind an abort or an init are given a bounded time to finish by drp_comm_destroy, drp_destroy and at exit. */
int drp_comm_unique_id(char* id128);                       /* ncclGetUniqueId */
/* ncclCommInitRank.  A ncclUniqueId serves one communicator per rank: a second drp_comm_init of the same (id, rank) in
 * this process returns DRP_ECOMM instead of never returning (several contexts of one process, one per GPU, share an id).
 * A rank whose peers do not arrive within DRP_COMM_INIT_TIMEOUT_S gets DRP_ECOMM; a communicator that comes up after that
 * is aborted by the helper that was waiting for it. */
int drp_comm_init(drp_ctx* ctx, const char* id128, int rank, int n_ranks);
int drp_comm_destroy(drp_ctx* ctx);
/* n_ranks = ncclCommCount and rank = ncclCommUserRank of the attached communicator (0 / -1 without one),
 * version = ncclGetVersion of the bound library, path = the file it was loaded from (each pointer nullable). */
int drp_comm_info(drp_ctx* ctx, int* n_ranks, int* rank, int* version, char* path, size_t path_len);
/* All-gather of one host buffer per rank over the context's communicator (upload, ncclAllGather, download):
 * recv [n_ranks][bytes] in rank order.  Without a communicator (or one rank) it copies send to recv.  The planner
 * mirror uses it for its per-iteration bookkeeping record (per-column best reward / index / pushes,
 * planners.py:721-727) when the sample axis is sharded; the update itself stays on the device. */
int drp_comm_allgather(drp_ctx* ctx, const void* send, size_t bytes, void* recv);

/* ---- resolution regressor (model/res_regressor.py:15-177) ---------------------------------------------------
 * The CNN the MPC loop asks for the particle count at every step (env/flex_env.py:981-998, :1083-1086; config/mpc/config.yaml:53-56
 * res_sel.active): five Conv2d(k=4, s=2, p=1) + LeakyReLU(0.2), 6 -> 64 -> 128 -> 256 -> 512 -> 512 channels, 224 -> 7 pixels,
 * NCHW flatten, Linear 25088 -> 4096 -> 1024 -> 256 -> 64 each + LeakyReLU(0.2), head Linear(64, n_out):
 * MPCResRgrNoPool (n_out 1, infer_param returns int(out)) or MPCResCls (n_out 6, [4, 8, 16, 32, 64, 128][argmax]).
 * Its weights and workspaces are the context's but apart from the PropNet's: loading or running one never touches the other.
 * Nothing is allocated before drp_rgr_load, which sizes every buffer for DRP_RGR_BMAX samples.  fp32 throughout; each output
 * element has one reduction order, fixed per layer and independent of B: a sample's outputs are bit-identical in any batch.
 * Each call runs on the context's stream and waits once, for its output copy. */
#define DRP_RGR_REGRESSOR 1     /* n_out of the MPCResRgrNoPool head */
#define DRP_RGR_CLASSIFIER 6    /* n_out of the MPCResCls head */
#define DRP_RGR_BMAX 64
#define DRP_RGR_SIZE 224        /* state_h = state_w */
/* blob: the state_dict model.{0,2,4,6,8,11,13,15,17,19}.{weight,bias} in that order, torch layouts, n_floats = 114 193 217
 * (n_out 1) or 114 193 542 (n_out 6); repacked on the device once (conv [Cout][kh][kw][Cin], FC1's columns in NHWC order). */
int drp_rgr_load(drp_ctx* ctx, const float* blob, size_t n_floats, int n_out);
/* x [B][6][224][224] (the stack of infer_param), 1 <= B <= DRP_RGR_BMAX -> out [B][n_out].  DRP_ESTATE before drp_rgr_load. */
int drp_rgr_forward(drp_ctx* ctx, const float* x, int B, float* out);
/* The stack of infer_param (model/res_regressor.py:146-175) from two [h][w] masks (nonzero = 1), h, w >= 224: the distance
 * transforms of 1 - mask (dt_mode DRP_DT_CV5 / DRP_DT_EXACT, both in one launch) over h, the two exclusions, each of the six
 * INTER_AREA-downscaled to 224 x 224 -> x_out [6][224][224] (nullable). */
int drp_rgr_stack(drp_ctx* ctx, const uint8_t* init, const uint8_t* goal, int h, int w, int dt_mode, float* x_out);
/* stack + forward at B = 1 -> out [n_out] (the caller applies int() or the argmax) */
int drp_rgr_infer(drp_ctx* ctx, const uint8_t* init, const uint8_t* goal, int h, int w, int dt_mode, float* out);
/* Device time of `iters` back-to-back forward passes at batch B on whatever the device buffers hold (measurement only):
 * parts = a sum of 1 (the convolutions), 2 (FC1: its GEMV and split-K reduction), 4 (FC2..head); ms_out [iters] (HIP events). */
int drp_rgr_time(drp_ctx* ctx, int parts, int B, int iters, float* ms_out);

/* ---- training the resolution regressor (train/train_res_rgr.py:100-222; loss and update :150-183) ----------------------
 * One step = the forward above (its outputs bit-identical to drp_rgr_forward's), the loss, the backward pass and Adam, on the
 * device.  Losses (the phase's `loss`, `mse` | `ce`, `reg`):
 *   regressor  (n_out 1): mse = mean_b conf[b] (out[b] - y[b])^2                (MSELoss(reduction='none')(out, y) * conf).mean()
 *   classifier (n_out 6): ce  = mean_b (logsumexp(out[b]) - out[b][label[b]])   CrossEntropyLoss()(out, label)
 *   reg  = sum |W| / n_W over the 10 weights (biases excluded; n_W = their element count), loss = mse|ce + lam_reg reg; its
 *          gradient lam_reg sign(W) / n_W with sign(0) = 0.
 * Optimiser: torch.optim.Adam(lr, betas=(beta1, 0.999)), eps 1e-8, no weight decay, over every parameter (k_adam's formula).
 * fp32 with float64 loss terms; every value has one fixed reduction order and there are no float atomics, so the same step
 * sequence gives bit-identical weights (gradients depend on B's split of the work, not on the run).
 * Memory: Adam's m and v (2 x 4 bytes per parameter) and the workspaces are allocated by drp_rgr_train_begin, the full
 * gradient buffer and its torch-layout staging copy only once a step asks for grad_out (then kept).  Nothing here touches the
 * PropNet weights or drp_train_* state. */
/* Allocates and zeroes Adam's state, t = 0.  DRP_ESTATE before drp_rgr_load; drp_rgr_load ends any training in progress. */
int drp_rgr_train_begin(drp_ctx* ctx, double lr, double beta1, double lam_reg);
/* x [B][6][224][224], 1 <= B <= DRP_RGR_BMAX; targets: y [B] and conf [B] for the regressor (label NULL), label [B] in 0..5
 * for the classifier (y, conf NULL); anything else is DRP_EINVAL.  mode DRP_TRAIN_EVAL (loss only), DRP_TRAIN_GRAD (the
 * weights stay as they are) or DRP_TRAIN_UPDATE (one Adam step).  loss_out [3] (nullable): loss, mse|ce, reg, always before
 * the update.  grad_out (nullable, DRP_TRAIN_GRAD only): the gradient, n_floats in state_dict order and torch layouts.
 * After an update drp_rgr_forward / drp_rgr_infer use the new weights.  DRP_ESTATE before drp_rgr_train_begin. */
int drp_rgr_train_step(drp_ctx* ctx, const float* x, const float* y, const float* conf, const int32_t* label, int B, int mode,
                       double* loss_out, float* grad_out);
int drp_rgr_train_set_lr(drp_ctx* ctx, double lr);
/* the device's weights back in the blob layout of drp_rgr_load (state_dict order, torch layouts) */
int drp_rgr_get_weights(drp_ctx* ctx, float* blob_out, size_t n_floats);
/* Device time of `iters` back-to-back UPDATE steps (they move the weights: measurement only) on the inputs of the last
 * drp_rgr_train_step, whose batch B must be: ms_out [iters][3] = forward | loss + FC backward with FC1's fused Adam step |
 * conv backward + Adam over the other parameters (HIP events). */
int drp_rgr_train_time(drp_ctx* ctx, int B, int iters, float* ms_out);

/* ---- GNN training batches from recorded episodes (row x4) ------------------------- */
/* ParticleDataset.__getitem__ (dataset/dataset_gnn_dyn.py:86-201) for B samples (1 <= B <= 1024) in one call, collated as
 * collate_fn (train/train_gnn_dyn.py:20-45) pads them.  Replaces, per sample: the depth PNG / (global_scale * 1000.0) and
 * depth2fgpcd (:97-98, utils.py:491-506, the float64 rule depth < 0.599/0.8 && depth > 0), fps_rad (:99, utils.py:438-449),
 * recenter in float64 with r = min(0.02, 0.5 / sqrt(den)) (:101, utils.py:468-477), the KDTree nearest-particle query
 * (:104-109: brute force in float64, the lowest index on an exact tie), the per-frame gather (:114-118) and the push formula
 * (:130-194).  Inputs: depth [B][h][w] uint16 (the PNGs as decoded), cam [fx, fy, cx, cy], T_cam = inv(opencv_T_world)
 * [4][4] row-major (:69-78), T = n_his + n_rollout frames; per sample b: n_ptcl[b] particles per frame, particles = the
 * samples' frames one after the other, [T][n_ptcl[b]][4] float32 each (FleX's world frame, column 3 ignored), radius[b] =
 * 1/sqrt(den), init_idx[b] = the sampler's start (numpy's randint(n_fg)), n_fg_host[b] = the foreground count the host drew
 * it from (the device's must agree), push [B][T-1][10] = s_3d_cam, e_3d_cam, push_dir_cam (unit), push_l in float64 as
 * :142-147 form them, episode (nullable) = the episode numbers errors name.  Outputs: states [B][T][n_max][3] and
 * states_delta [B][T-1][n_max][3] float32, zero beyond each count (room for n_cap particle slots), counts_out [B],
 * *n_max_out.  DRP_EINVAL (the context stays usable) for an empty foreground, a count that disagrees, a zero-length push or
 * one with |push_dir_cam z| >= 1e-6, a sample that reaches 4096 particles, bad shapes.  Own workspaces: nothing of the
 * PropNet, training, planning or regressor state is touched.  One wait after the sampler (the counts), one at the end. */
int drp_ptcl_dataset_batch(drp_ctx* ctx, int B, const uint16_t* depth, int h, int w, double global_scale, const double cam[4],
                           const double T_cam[16], int T, const int32_t* n_ptcl, const float* particles, const double* radius,
                           const int32_t* init_idx, const int32_t* n_fg_host, const double* push, const int32_t* episode,
                           int n_cap, float* states_out, float* sdelta_out, int32_t* counts_out, int* n_max_out);
/* Untracked samples straight from recorded depth frames (row x4 / u1): the chain depth PNG / (global_scale * 1000.0) ->
 * depth2fgpcd -> fps_rad -> recenter (dataset/dataset_gnn_dyn.py:97-101, utils.py:491-506, 438-449, 468-477) on EVERY frame of B
 * windows of T frames, T >= 1 and 1 <= B * T <= 1024 images per call; no particle file is involved.  Frame 0 of a window is
 * the state a Chamfer + actions training step starts from, frames 1..T-1 are its target clouds, each with its own count.
 * Inputs: depth [B][T][h][w] uint16, cam [fx, fy, cx, cy]; per (sample, frame): radius[b][t] (fps_rad's; recenter uses r =
 * min(0.02, 0.5 * radius[b][t])), init_idx[b][t] = the sampler's start (numpy's randint(n_fg)), n_fg_host[b][t] = the foreground
 * count the host drew it from (the device's must agree); episode [B] (nullable) = the episode numbers errors name.  Outputs:
 * clouds [B][T][n_max][3] float32 = each recentered float64 point rounded once, +0.0f beyond counts_out[b][t] (room for n_cap
 * particle slots per frame); *n_max_out = the largest count of the call.  float64 in the reference's evaluation order, no
 * atomics: frame t of a window has the bits a T = 1 call on that frame has, frame 0 those of drp_ptcl_dataset_batch's sampler
 * and recenter on the same sample and draws.  DRP_EINVAL (the context stays usable; the message names episode and frame) for a
 * null argument or bad shapes, B * T out of range, a non-positive or non-finite radius, a frame without foreground, a host
 * count that disagrees, a start outside its cloud, a frame that reaches 4096 particles, n_max > n_cap.
 * Memory: the upload is 2 * B * T * h * w bytes (pinned staging and its device copy), the clouds and the sampler's distances
 * 32 * sum(n_fg) bytes: about 1.6 GB of device memory for 64 samples x 6 frames at 720 x 720 with 90 k foreground pixels --
 * hence the image limit.  Workspaces: drp_ptcl_dataset_batch's (the two calls share them and one pinned staging block for
 * both directions); nothing of the PropNet weights, a training / planning session, the regressor or drp_obs2ptcl is touched.
 * One wait after the sampler (the counts), one at the end. */
int drp_ptcl_dataset_frames(drp_ctx* ctx, int B, int T, const uint16_t* depth, int h, int w, double global_scale,
                            const double cam[4], const double* radius, const int32_t* init_idx, const int32_t* n_fg_host,
                            const int32_t* episode, int n_cap, float* clouds_out, int32_t* counts_out, int* n_max_out);
/* Device time of the last completed drp_ptcl_dataset_batch or drp_ptcl_dataset_frames, whichever completed last, by stage (HIP
 * events): ms_out [6] = upload | compaction | fps_rad | recenter | track + pack (frames: the pack alone) | download.
 * DRP_ESTATE before the first. */
int drp_ptcl_dataset_time(drp_ctx* ctx, float* ms_out);

/* ---- measurement / debugging ----------------------------------------------------- */
/* HIP-event timing of one kernel class on the context's stream.  name: "graph",
 * "node_encode", "edge_encode", "project", "aggregate", "update", "predict", "reward",
 * "mppi", "prop" (the fused propagation-step kernel of DRP_ENGINE_FUSED / _LITE), "loss" (the stand-alone metrics' kernel:
 * drp_cloud_chamfer, drp_cloud_match, drp_cloud_transport, drp_cloud_divergence, drp_cloud_divergence_unbalanced, drp_cloud_divergence_f64, drp_cloud_divergence_unbalanced_f64, drp_cloud_match_f64).  drp_probe_read returns total ms and launches since drp_probe_begin. */
int drp_probe_begin(drp_ctx* ctx, const char* kernel_class);
int drp_probe_read(drp_ctx* ctx, double* total_ms, long* launches);
/* Kernel launches inside the timed regions of the "prop" / "prop+work" probe since drp_probe_begin.  drp_probe_read's `launches`
 * counts regions, and a region of the whole-sample kernels covers one launch per block of samples (csrc/dispatch.h: cut_blocks):
 * a batch that is cut into blocks shows here.  Reading does not reset the count; 0 while another class is probed. */
int drp_probe_prop_launches(drp_ctx* ctx, long* kernels);
/* What the propagation kernels (km_prop, km_prop3, km_rollout) EXECUTED since drp_probe_begin(ctx, "prop+work") -- the "prop"
 * probe with the kernels' own counters switched on (two atomic adds per tile: they cost the 300-particle launch 8 %, so a
 * timed region runs under the plain "prop" probe and the counters over an iteration of their own): out[0] slot iterations that ran the relation
 * encoder's chain (78 16-bit MFMAs each), [1] slot iterations served by the edge-chain cache (none), [2] / [3] tiles of
 * propagation steps that are not / are the last (144 / 96), [4] particle-encoder tiles inside the launch (204),
 * [5] the 16-bit MFMAs (32x32x16, 32 768 FLOP each) those add up to, by the engine the counted launches ran on: on
 * DRP_ENGINE_LITE the units weigh 26, 72 / 48 and 102 (count one engine per drp_probe_begin: DRP_ESTATE otherwise); [6] shader-clock cycles (s_memtime) and [7] 100 MHz
 * ticks (s_memrealtime) between entry and exit of the counted launches, summed over their workgroups: 100 * [6] / [7] is the
 * shader clock in MHz the kernel ran at.  bench.py's roofline numerator and its sclk_mhz_under_load. */
int drp_probe_work(drp_ctx* ctx, unsigned long long out[8]);
/* Which kernel variant served the launches since drp_dispatch_reset (or drp_create): graph build (k_graph, k_graph_q4,
 * k_graph_strips_q<128|256>, k_graph_cells, k_graph_rev, inside km_rollout), propagation kernel with its template flags
 * (km_prop<last|mid,tape,pair,work>, km_prop3<tape|plain,pair,cache|cache+rows,work>, km_rollout<pair|tile32,...>), the
 * stage kernels of the fp32 engines, reverse-mode variant (kmb_rows_bwd, kmb_step_bwd, the stage kernels), training and
 * pre-processing kernels -- names joined by ';' into out (truncated to out_len), return value = the full length.
 * drp_dispatch_variants lists every name the library can report (default_only != 0: without those that need an environment
 * switch or the counting probe).  The shapes and thresholds that select a variant are measured constants
 * (csrc/capi_ctx.h, capi_pipeline.h); tests/test_gpu_fuzz_oracle.py checks every default variant against the oracle through these. */
int drp_dispatch_reset(drp_ctx* ctx);
long drp_last_dispatch(drp_ctx* ctx, char* out, size_t out_len);
long drp_dispatch_variants(int default_only, char* out, size_t out_len);
/* The split-fp16 relation encoder's range shift for the loaded weights: hidden activations travel as two fp16 pieces
 * times 2^-shift; bound = the proven largest activation for the envelope |attr| <= 2, |s_r - s_s| <= 1.5, density <= 10 000;
 * wmax = the largest |weight| packed as fp16; ok = 0 when no shift can carry the weights (every call of the fused / split
 * engine then returns DRP_ERANGE; the gradient-descent planner and the trainer write their tape on the fp32 engine).
 * Each pointer nullable. */
int drp_range_info(drp_ctx* ctx, int* shift, double* bound, double* wmax, int* ok);
/* hold the context's stream for ms (<= 10 000) milliseconds -- what a collective waiting for a dead peer looks like to
 * the host; the tests of the hang guard use it */
int drp_debug_stall(drp_ctx* ctx, int ms);
/* copy an intermediate device buffer to the host: "s_delta","nbr_idx","nbr_cnt",
 * "particle_encode"(eff0),"c_node","c_edge","proj","agg","effect"; the weight blob "w_raw" and its packed copies
 * "w_valu","w_mfma","w_mfma_bwd","w_split","w_split6"; the resolution regressor's post-activation taps of its last forward
 * "rgr_c1".."rgr_c5" (NHWC [B][H][W][C]) and "rgr_f1".."rgr_f4" ([B][features]); the last drp_ptcl_dataset_batch's
 * "pd_nfg" ([B] int32), "pd_chosen" ([B][4097] int32), "pd_recenter" ([B][n_max][3] float64), "pd_nearest" ([B][n_max]
 * int32); the last drp_ptcl_dataset_frames's "pdf_nfg" ([B][T] int32), "pdf_chosen" ([B][T][4097] int32), "pdf_recenter"
 * ([B][T][n_max][3] float64).  The two dataset calls share their buffers: a "pd_*" tap after a frames call, or a "pdf_*" tap
 * after a batch call, is DRP_ESTATE (not populated), never the other call's bytes.  The last trainer call's "train_states"
 * ([B][H][N][3] float32, the predicted states), "train_sdelta" ([H][B][N][3], the impulses) and "train_seed" ([H][B][N][3]
 * float32: d loss / d s_pred as the call's loss kernel left it -- the loss's own seed after a call with DRP_TRAIN_EVAL, which runs
 * no reverse pass over it; a reverse pass adds the later steps' shares to every slice but the last).  The tape's lists of every
 * step: "train_nbr_idx", "train_nbr_cnt", "train_rev_off", "train_rev".
 * The weight-gradient sums of the last trainer call that ran a reverse pass with deferred weight gradients (the default), read-only:
 * "train_wgrad_jobs" -- one record of 11 int64 per job of the pass, in queue order: M, in, rows_per_sample, dens_mod, blocks,
 * lane_stride, k_stride, the offsets in floats of dW, db and dwd inside the gradient blob (-1: none), whether the densities are read;
 * then one more record for the column sums of the predictor's last bias (M, in = 3, its target as the db offset; the rest 0 / -1).
 * dW[lane * lane_stride + k * k_stride] += sum_rows g[row][lane] x[row][k] (k < in), db[lane] += sum_rows g[row][lane],
 * dwd[lane * lane_stride] += sum_rows g[row][lane] (dens[(row / rows_per_sample) % dens_mod] / 5000 in fp32).  "train_wgrad_g:<q>" and
 * "train_wgrad_x:<q>" -- job q's operand rows as dense [M][64] / [M][in] float32 (whatever the strides in device memory are); the
 * column sums' rows [M][3] under "train_wgrad_g:<number of jobs>".  "train_wgrad_dens" -- the densities [dens_mod] the jobs read.
 * No device pointer leaves.  DRP_ESTATE (not populated) after a pass that did not defer (DRP_NO_WGRAD_DEFER=1, or operands beyond
 * 8 GB), after DRP_TRAIN_EVAL or drp_train_predict, after a trainer call that failed, and after any later call that stages a step's
 * inputs (they share the buffers); DRP_EINVAL for an index the pass did not queue.  drp_train_accumulate and drp_train_apply leave
 * the taps valid.  (byte sizes: the returned value). returns bytes. */
long drp_debug_fetch(drp_ctx* ctx, const char* name, void* out, size_t out_bytes);

/* ---- the float64 yardstick: one step evaluated in double on the device, and a probe that holds an engine against it ----
 * Not a value of drp_set_engine: it has no dispatch plan and leaves no trace in drp_last_dispatch.  It stages in buffers of
 * its own, so none of these calls ends a planner session, and none changes the engine drp_set_engine selected.
 *
 * PropModuleDiffDen.forward (model/gnn_dyn.py:147-198) in float64, relations as lists (as drp_forward); the inputs are the
 * fp32 values widened exactly, the weights the loaded fp32 blob widened exactly (after a training step: the updated blob).
 * The reference's own formulation -- relation propagator over cat[relation_encode, effect_r, effect_s, dens] (:186-187),
 * particle propagator over cat[particle_encode, agg, dens] with the residual inside the ReLU (:191-193, :82-85) -- on
 * v_mfma_f64_16x16x4_f64.  One reduction order per output (ascending k, ascending slot), no atomics: a sample's result is
 * the same bits alone, in any batch and from run to run.  The batch is walked in sample chunks under a workspace cap
 * (256 MB; 24 KB of float64 intermediates per particle), which changes no bit.  Shape limits as drp_forward; a list entry
 * outside 0..N-1 or a count above 10 is DRP_EINVAL.  s_pred_out [B,N,3] double. */
int drp_forward_f64(drp_ctx* ctx, const float* a_cur, const float* s_cur, const float* s_delta, const float* dens,
                    const int16_t* nbr_idx, const uint8_t* nbr_cnt, int B, int N, double* s_pred_out);
/* predict_one_step (model/gnn_dyn.py:209-254): the lists from the library's own fp32 graph build (bit-exact with the
 * reference's, :223-251), then the above. */
int drp_step_f64(drp_ctx* ctx, const float* a_cur, const float* s_cur, const float* s_delta, const float* dens, int B, int N,
                 double* s_pred_out);
/* The float64 intermediates of the last drp_forward_f64 / drp_step_f64 / drp_accuracy_probe, n doubles (exactly the tap's size):
 * "particle_encode" [B,N,64] (:174; also answered as "c_node"), "relation_encode" [B,N,10,64] (:179, receiver-major slots,
 * zeros past a receiver's count; also "c_edge"), and for the propagation steps p = 0..2 "effect_rel_p" [B,N,10,64] (:186),
 * "agg_p" [B,N,64] (:189), "effect_p" [B,N,64] (:191; also "particle_effect_p"); "particle_pred" [B,N,3] (:196).
 * DRP_ESTATE when that call walked its batch in more than one chunk. */
int drp_f64_tap(drp_ctx* ctx, const char* name, double* out, size_t n);
/* the workspace cap of the *_f64 calls in bytes (0: the default, 256 MB); one sample is the smallest chunk.  Tests lower it
 * to force chunking. */
int drp_debug_set_f64_cap(drp_ctx* ctx, size_t bytes);
/* drp_step's path on `engine` (DRP_ENGINE_*, any of the five) and drp_step_f64 on the same inputs and the same lists, reduced
 * on the device: out[0] = max |s_pred_engine - s_pred_f64| (the fp32 value widened, the difference in double),
 * out[1] = max |s_pred_f64 - s_cur|, out[2] = out[0] / max(out[1], 1e-12) (the error as a share of the largest displacement,
 * the quantity the 1e-4 parity tolerance is stated in), out[3] = index b * N + n of the worst particle (ties: the lowest).
 * A refusal of the engine (DRP_ERANGE) is returned as such. */
int drp_accuracy_probe(drp_ctx* ctx, int engine, const float* a_cur, const float* s_cur, const float* s_delta,
                       const float* dens, int B, int N, double out[4]);

/* ---- the float64 yardstick of the gradient (row y2): what drp_gd_begin + drp_gd_grad compute (planners.py:685-745: row =
 * traj * nb + batch, an H-step rollout, the final step's config_reward_ptcl, loss = -sum reward, reverse mode through every
 * step), every product and sum in double.  A one-shot call: no drp_gd_begin, no session begun or ended, buffers of its own,
 * the selected engine, drp_last_dispatch and the degree statistic as before; taps of an earlier *_f64 call stay answered.
 * Camera, goal field and goal points are the context's, the weights the float64 copy of the loaded blob, all widened exactly.
 * Forward: gen_s_delta (planners.py:211-257, hard mask included, with its constants 0.8 / 24 and 0.01 as the reference's
 * expressions give them in double) on the double state; the step's lists from the library's own fp32 graph build on the fp32
 * roundings of that state and impulse (as drp_step_f64); the step as drp_forward_f64, its intermediates kept as the tape; the
 * next state stays in double.  The reward (env/flex_rewards.py:189-214) in double: projection, grid_sample's border clamp and
 * floor-chosen bilinear cell, one-sided chamfer with the lowest particle index winning a tie.  Backward: graph, hard mask,
 * bilinear cell and arg-min are constants, as autograd treats them.  64-wide blocks on v_mfma_f64_16x16x4_f64; ONE reduction
 * order per value (ascending k, ascending slot, the sender scatter as a gather over reversed lists in ascending edge order),
 * no atomics: a row's outputs are the same bits alone, in any batch, from run to run and under any workspace cap
 * (drp_debug_set_f64_cap: the batch is walked in row chunks, tape 24 KB per particle and step; one row is the smallest chunk).
 * rewards_out [B], grad_act_out [B,H,4] = d loss / d pushes, grad_state_out [B,H,N,3] = d loss / d every step's predicted state
 * (as drp_gd_grad); each nullable.  DRP_ESTATE without weights, camera or goal; DRP_EINVAL for non-positive sizes, H > 64, B
 * not a multiple of nb, N beyond drp_forward's limit.  A zero-length push gives NaN, as the reference. */
int drp_gd_grad_f64(drp_ctx* ctx, const float* s0, const float* attr, const float* dens, int nb, int N, const float* actions,
                    int B, int H, double* rewards_out, double* grad_act_out, double* grad_state_out);
/* The float64 yardstick of drp_gd_predict / drp_gd_grad_seeded: the same tape and reverse pass with the caller's seed [B][H][N][3]
 * (doubles) in the reward's place, joined at the point drp_gd_grad_seeded documents.  One-shots with drp_gd_grad_f64's contract
 * (no session begun or ended, buffers of their own, chunked under drp_debug_set_f64_cap with the seed sliced per chunk, the same
 * bits run to run and under any cap), but they need no goal.  states_out [B][H][N][3]; grad_act_out, grad_state_out as
 * drp_gd_grad_f64's, nullable.  DRP_EINVAL for a null seed / states_out or a seed value that is infinite or not a number. */
int drp_gd_predict_f64(drp_ctx* ctx, const float* s0, const float* attr, const float* dens, int nb, int N, const float* actions,
                       int B, int H, double* states_out);
int drp_gd_grad_f64_seeded(drp_ctx* ctx, const float* s0, const float* attr, const float* dens, int nb, int N, const float* actions,
                           int B, int H, const double* seed, double* grad_act_out, double* grad_state_out);

/* ---- the float64 yardstick of the trainer's gradients (row y3): what drp_train_step(mode = DRP_TRAIN_GRAD) computes
 * (train/train_gnn_dyn.py:167-203; layouts as there: states [B, n_rollout+1, N, 3], states_delta [B, n_rollout, N, 3], attrs
 * [B, n_rollout+1, N], particle_nums [B], particle_dens [B]), every product and sum in double.  A one-shot call: no
 * drp_train_begin (n_rollout is an argument), no session begun or ended, buffers of its own; the selected engine,
 * drp_last_dispatch, the degree statistic, the trainer's Adam moments, iteration count, learning rate and launch plan, and the
 * taps of an earlier *_f64 call are as before.  The weights are the float64 copy of the current blob (after an optimiser step:
 * the updated one), the inputs widened exactly.
 * Forward: s_cur = states[:, 0], a_cur = attrs[:, 0]; each step's impulse is states_delta[:, t]; its lists come from the
 * library's own fp32 graph build, in the trainer's mode for zero-padded batches, on the fp32 roundings of the double state; the
 * step as drp_forward_f64, its intermediates kept as the tape; s_cur <- s_pred stays in double.  loss_terms_out [n_rollout][B] =
 * mse(s_pred[b, :n_b], states[b, t+1, :n_b]) / (n_rollout B) as float64 sums of squared double differences; loss_out = their
 * sum, step-major.  Backward: drp_gd_grad_f64's kernels, the state gradient seeded by 2 (s_pred - s_nxt) / (3 n_b n_rollout B)
 * on real rows and 0 on padded ones; the impulse is data; the graph is a constant.  Weight gradients dW = G^T X: the 64-wide
 * blocks on v_mfma_f64_16x16x4_f64 with the rows as the k dimension (the receiver's and sender's effects gathered through the
 * lists inside the load), the narrow inputs, density columns and biases as one ascending chain per entry; a slot past its
 * receiver's count contributes exactly zero.  ONE reduction order per value, no atomics: (sample, step) contributions in
 * ascending row order, added per sample in the order the reverse pass visits the steps, the samples in ascending order in one
 * chain per entry -- grad_out is the same bits from run to run and under any workspace cap (drp_debug_set_f64_cap: sample
 * chunks; tape 24 KB per particle and step, 307 KB of accumulators per sample; one sample is the smallest chunk).
 * grad_out: 38 403 doubles in state_dict order; grad_state_out [B, n_rollout, N, 3] = d loss / d every step's predicted state;
 * each output nullable.  DRP_ESTATE without weights; DRP_EINVAL for non-positive sizes, n_rollout > 64, N beyond drp_forward's
 * limit, a particle_nums[b] outside 1..N, null inputs. */
int drp_train_grad_f64(drp_ctx* ctx, const float* states, const float* states_delta, const float* attrs,
                       const int32_t* particle_nums, const float* particle_dens, int B, int N, int n_rollout,
                       double* loss_out, double* loss_terms_out, double* grad_out, double* grad_state_out);
/* drp_train_grad_f64 with actions [B, n_rollout, 4] in place of states_delta: the yardstick of drp_train_step_actions' gradients
 * with the MSE loss (train/train_gnn_dyn.py:159-189 with planners.py:211-257 evaluated at s_cur, in double).  Step t's impulse is
 * drp_gd_grad_f64's gen_s_delta on the double state, zero on rows n >= particle_nums[b]; for t > 0 the push's position share
 * (hard mask constant, soft mask and projections differentiated) joins d loss / d s_pred_{t-1} on real rows.  Everything else,
 * the one-shot contract included, is drp_train_grad_f64's.  DRP_ESTATE also without a camera; DRP_EINVAL also for a push of
 * zero length.  (The Chamfer loss on the same pushes: drp_train_grad_f64_untracked below.) */
int drp_train_grad_f64_actions(drp_ctx* ctx, const float* states, const float* actions, const float* attrs,
                               const int32_t* particle_nums, const float* particle_dens, int B, int N, int n_rollout,
                               double* loss_out, double* loss_terms_out, double* grad_out, double* grad_state_out);
/* drp_train_grad_f64 (states_delta given, actions NULL) or drp_train_grad_f64_actions (actions given, states_delta NULL) with the
 * Chamfer loss of drp_train_step_untracked in place of the MSE: the yardstick of drp_train_step_untracked's and of
 * drp_train_step_actions' (with targets) gradients, row u1.  The term of (step t, sample b) is (fwd + bwd) / (n_rollout B) of
 * drp_cloud_chamfer_f64 below between the DOUBLE prediction s_pred_t[b, :n_b] and targets[b, t, :target_nums[b, t]] widened
 * exactly; it seeds the reverse pass with its gradient on real rows and +0.0 on padded ones, and everything behind the seed is
 * drp_train_grad_f64's code.  The arg-mins are taken in double on the double prediction (lowest index on a tie) and are constants
 * of the derivative: unlike the graph lists, which come from the fp32 build, the fp32 trainer's arg-mins are no input here.  A
 * near-tie can therefore give the fp32 tape another partner than this call, which moves a gradient by a discrete amount and is
 * no arithmetic error: margin_out [n_rollout][B] (nullable) is, per (step, sample), the smallest (second-best - best) squared
 * distance over all its arg-mins of both directions -- 0 for a duplicate of a winner, +inf where every other cloud has one row.
 * Of states only step 0 is read.  The same bits from run to run and under any workspace cap.  The one-shot contract is
 * drp_train_grad_f64's; it is no dispatch variant.  Refusals: those of drp_train_grad_f64 / drp_train_grad_f64_actions, and
 * DRP_EINVAL unless exactly one of states_delta and actions is given, for null targets or target_nums, M outside 1..4096, a
 * target_nums entry outside 1..M.  A refused call leaves the context usable. */
int drp_train_grad_f64_untracked(drp_ctx* ctx, const float* states, const float* states_delta /*[B][H][N][3] or NULL*/,
                                 const float* actions /*[B][H][4] or NULL*/, const float* attrs, const int32_t* particle_nums,
                                 const float* particle_dens, int B, int N, int n_rollout,
                                 const float* targets /*[B][H][M][3]*/, const int32_t* target_nums /*[B][H]*/, int M,
                                 double* loss_out, double* loss_terms_out, double* grad_out, double* grad_state_out,
                                 double* margin_out /*[H][B], nullable*/);

/* ---- symmetric squared Chamfer distance of two padded cloud batches and its gradient; no counterpart in the reference
 * (env/flex_rewards.py:9 imports pytorch3d's and never uses it).  p [B][N][3] with n_p[b] real rows, q [B][M][3] with n_q[b];
 * rows beyond a count are padding: never read as points, gradient exactly 0, neighbour -1.
 *   a(i) = argmin_j |p_i - q_j|^2  j < n_q (lowest j on a tie)      c(j) = argmin_i |q_j - p_i|^2  i < n_p (lowest i on a tie)
 *   fwd = 1/(3 n_p) sum_i |p_i - q_a(i)|^2                          bwd = 1/(3 n_q) sum_j |q_j - p_c(j)|^2
 *   d (fwd + bwd) / d p_i = 2/(3 n_p) (p_i - q_a(i)) + 2/(3 n_q) sum_{j: c(j) = i} (p_i - q_j)       (arg-mins constant)
 * The 1/3 is the per-coordinate mean of F.mse_loss: where the nearest neighbour is the true partner, fwd is the tracked loss's
 * MSE term.  Squared distances in fp32 from fp32 differences, the sums in double, no atomics: the same bits from run to run and
 * for a sample alone or inside any batch.  A one-shot (the three drp_cloud_* calls share one buffer; each ends in a wait and
 * keeps nothing between calls): needs no weights, ends no drp_mpc_* / drp_gd_* /
 * training session, leaves the selected engine, drp_last_dispatch and the trainer's state alone.  DRP_EINVAL: a null argument
 * (the last three outputs are nullable), a count outside 1..N or 1..M, N or M outside 1..4096. */
int drp_cloud_chamfer(drp_ctx* ctx, const float* p, const int32_t* n_p, const float* q, const int32_t* n_q,
                      int B, int N, int M, double* terms_out /*[B][2]: fwd, bwd*/,
                      float* grad_p_out /*[B][N][3], nullable; scale = 1*/,
                      int32_t* nn_pq_out /*[B][N], nullable*/, int32_t* nn_qp_out /*[B][M], nullable*/);
/* drp_cloud_chamfer in float64, the yardstick of the metric: p and q widened exactly, a squared distance dx*dx + dy*dy + dz*dz
 * in double in that order without fused multiply-add, the arg-mins taken in double (strict <, lowest index on a tie), sums and
 * gradient in double in one fixed order, no atomics.  margin_out [B][2] (nullable): the smallest (second-best - best) squared
 * distance over the real rows' arg-mins, p -> q then q -> p; 0 exactly for a duplicate of a winner, +inf where the other cloud
 * has one row.  Contract and refusals are drp_cloud_chamfer's. */
int drp_cloud_chamfer_f64(drp_ctx* ctx, const float* p, const int32_t* n_p, const float* q, const int32_t* n_q,
                          int B, int N, int M, double* terms_out /*[B][2]: fwd, bwd*/,
                          double* grad_p_out /*[B][N][3], nullable; scale = 1*/,
                          int32_t* nn_pq_out /*[B][N], nullable*/, int32_t* nn_qp_out /*[B][M], nullable*/,
                          double* margin_out /*[B][2]: p -> q, q -> p; nullable*/);

/* ---- one-to-one matching (earth mover's) distance of two padded cloud batches and its gradient: what the Chamfer
 * distance is blind to -- any number of predicted rows may share one nearest target there, here every row of the smaller cloud
 * has a partner of its own.  p, q, the counts and the padding as drp_cloud_chamfer; r = min(n_p, n_q).
 *   C[i][j] = |p_i - q_j|^2 in fp32, formed as drp_cloud_chamfer forms it (fp32 differences, dx*dx + dy*dy + dz*dz, no fma)
 *   sigma   = the matching of every row of the SMALLER cloud to a distinct row of the larger one that minimises sum C (the
 *             rectangular linear assignment problem; the exact optimum by shortest augmenting paths with duals, shortest
 *             distances and reduced costs in double -- no epsilon)
 *   match   = sum_pairs |p_i - q_j|^2 / (3 r), each pair's squared fp32 differences summed in double.  With n_p = n_q and the
 *             matching the tracked correspondence this is the tracked loss's MSE term.
 *   d match / d p_i = 2 (p_i - q_sigma(i)) / (3 r) for a matched row; +0.0 exactly for a row left unmatched (n_p > n_q) and for
 *             padding.  sigma is a constant of the derivative.
 * Deterministic: rows of the smaller cloud (p's where n_p = n_q) are inserted in ascending index, among equal shortest reduced
 * costs the lowest column index wins, nothing is atomic -- the same bits from run to run and for a sample alone or inside any
 * batch.  match_pq_out [B][N] / match_qp_out [B][M]: the partner's index, -1 for unmatched rows and padding.  dual_out
 * [B][N + M]: the duals of p's rows, then of q's (0 on padding): u_i + v_j <= C[i][j], equal on matched pairs, 0 on the larger
 * cloud's unmatched rows, sum u + sum v = sum_pairs C.  N and M are at most 1024 (the work is r^2 dependent steps of c / 64
 * each); the kernel's loops are counted by r and c alone, whatever the values.  Contract as drp_cloud_chamfer: a one-shot
 * that needs no weights, ends no session and leaves the engine, drp_last_dispatch and the trainer alone.
 * DRP_EINVAL: a null argument (every output but terms_out is nullable), a count outside 1..N or 1..M, N or M outside 1..1024, a
 * real row that is not finite. */
int drp_cloud_match(drp_ctx* ctx, const float* p, const int32_t* n_p, const float* q, const int32_t* n_q,
                    int B, int N, int M, double* terms_out /*[B]*/, float* grad_p_out /*[B][N][3], nullable*/,
                    int32_t* match_pq_out /*[B][N], nullable*/, int32_t* match_qp_out /*[B][M], nullable*/,
                    double* dual_out /*[B][N+M], nullable*/);

/* The loop body of train/train_gnn_dyn.py:159-189 with the loss of each step chosen by argument: drp_train_step_untracked
 * (states_delta given, actions NULL) or drp_train_step_actions (actions given, states_delta NULL) -- exactly one of the two --
 * against targets [B][H][M][3] with target_nums [B][H], and
 *   DRP_LOSS_CHAMFER        the Chamfer term: the bits of drp_train_step_untracked / drp_train_step_actions
 *   DRP_LOSS_MATCH          the matching term of drp_cloud_match between s_pred_t[b, :n_b] and targets[b, t, :target_nums[b, t]],
 *                           / (n_rollout B)
 *   DRP_LOSS_CHAMFER_MATCH  (1 - w) (fwd + bwd) + w match with w = match_weight in (0, 1): the Chamfer kernel runs first and leaves
 *                           a Chamfer-only step's terms and state gradient, the matching kernel behind it in the stream turns
 *                           each into (1 - w) x it + its own share, in double, rounded once: one writer per element, a fixed
 *                           order, and the loss is (1 - w) x the Chamfer call's + w x the matching call's to double rounding
 * match_weight is read by the mix only.  match_out [H][B][N] (nullable; kinds with a matching): the partner in the target of every
 * predicted row, per (step, sample), -1 for an unmatched row and padding.  Everything behind the loss gradient is
 * drp_train_step's; it is no dispatch variant.  A diverged model's non-finite prediction ends in a NaN loss after the same
 * number of steps.  Refusals (the context stays as it was): those of the call it generalises; N or M above 1024 with a matching;
 * match_weight outside (0, 1) for the mix; both or neither of states_delta and actions; another loss_kind. */
#define DRP_LOSS_CHAMFER 1
#define DRP_LOSS_MATCH 2
#define DRP_LOSS_CHAMFER_MATCH 3
int drp_train_step_loss(drp_ctx* ctx, const float* states, const float* states_delta /*or NULL*/, const float* actions /*or NULL*/,
                        const float* attrs, const int32_t* particle_nums, const float* particle_dens, int B, int N,
                        const float* targets /*[B][H][M][3]*/, const int32_t* target_nums /*[B][H]*/, int M, int loss_kind,
                        double match_weight, int mode, double* loss_out, float* grad_out, int32_t* match_out /*[H][B][N], nullable*/);

/* ---- entropy-regularised optimal-transport distance of two padded cloud batches and its gradient: transport with
 * fractional masses, where clouds of unequal counts share mass instead of leaving rows unmatched.  The inputs are a prediction p
 * with n_p real rows and a target q with n_q real rows; padding is as for drp_cloud_chamfer.
 *   Cost.        C[i][j] is the fp32 squared distance exactly as kc_chamfer forms it: fp32 differences, dx*dx + dy*dy + dz*dz,
 *                no fma.  It is widened to double exactly.  Everything after it is double.
 *   Masses.      a_i = 1/n_p, b_j = 1/n_q.
 *   Parameters.  eps = eps[b] > 0 is in squared-distance units, per sample.  K = iters satisfies 1 <= K <= KT_MAX_ITERS
 *                (DRP_TRANSPORT_MAX_ITERS).
 *   Sweeps.      f = 0.  For k = 1 .. K, first g_j = -eps LSE_i((f_i - C_ij)/eps + log a_i), then
 *                f_i = -eps LSE_j((g_j - C_ij)/eps + log b_j).  LSE is max-shifted.  Its terms are added in a fixed order that
 *                DESIGN.md 9 states (ascending index within each of the lanes that share a sum, then an xor butterfly over
 *                those lanes).  The last update is f's, so the plan P_ij = a_i b_j exp((f_i + g_j - C_ij)/eps) has row sums a_i
 *                to rounding.  Every predicted particle's whole mass is placed.
 *   Term.        transport = sum_ij P_ij C_ij / 3.  This is the same /3 as match.  With equal counts and eps -> 0 it tends to
 *                the match term.
 *   Gradient.    d/dp_i = scale sum_j P_ij 2 (p_i - q_j) / 3.  P is a constant of the derivative, as sigma is for match.  The
 *                differences are the fp32 ones.  The sum is in double and is rounded once to fp32.  The gradient is +0.0 exactly
 *                on padding.
 *   col_err.     col_err = sum_j |sum_i P_ij - b_j| is the column-marginal violation that K sweeps leave.  It is the caller's
 *                certificate that K was enough.  It is an output, not a stopping rule.
 *   Fixed work.  The loops are counted by K, n_p and n_q alone.  No value prolongs them.
 *   Non-finite input.  The stand-alone call refuses a non-finite real row on the host.  In the trainer a non-finite prediction
 *                ends in a NaN loss after the same number of steps.
 *   Determinism. No atomics.  The bits are the same from run to run.  They are the same for a sample alone or inside any batch.
 *                They do not depend on the padded N and M, only on the counts.
 * dual_out [B][N + M]: f then g, 0 on padding.  N and M are at most 1024 (the work is K n_p n_q exponentials).  Contract as
 * drp_cloud_match: a one-shot that needs no weights, ends no session, is no dispatch variant and leaves drp_last_dispatch and the
 * trainer alone; it counts under the "loss" kernel class of drp_probe_begin.
 * DRP_EINVAL (the context stays usable): a null argument (every output but terms_out is nullable), a count outside 1..N or 1..M, N
 * or M outside 1..1024, eps[b] not finite or <= 0, iters outside 1..DRP_TRANSPORT_MAX_ITERS, a real row that is not finite. */
#define DRP_TRANSPORT_MAX_ITERS 1000
int drp_cloud_transport(drp_ctx* ctx, const float* p, const int32_t* n_p, const float* q, const int32_t* n_q,
                        int B, int N, int M, const double* eps /*[B]*/, int iters, double* terms_out /*[B]*/,
                        float* grad_p_out /*[B][N][3], nullable*/, double* dual_out /*[B][N+M]: f then g, nullable*/,
                        double* col_err_out /*[B], nullable*/);

/* drp_train_step_loss's body with the transport term of drp_cloud_transport between s_pred_t[b, :n_b] and
 * targets[b, t, :target_nums[b, t]] as each step's loss, / (n_rollout B); eps [B] (per sample, every step of it) and iters as
 * there.  states_delta or actions: exactly one of the two.  The transport kernel is launched where the Chamfer kernel is and
 * writes the same state gradient, loss terms and zero-fill; everything behind the loss gradient is drp_train_step's; it is no
 * dispatch variant.  col_err_out [H][B] (nullable): every problem's col_err.  A call of its own because drp_train_step_loss has no
 * room for eps and iters: that call's accepted kinds stay 1..3.  Refusals (the context stays as it was): those of
 * drp_train_step_loss; N or M above 1024; a null eps, eps[b] not finite or <= 0; iters outside 1..DRP_TRANSPORT_MAX_ITERS. */
int drp_train_step_transport(drp_ctx* ctx, const float* states, const float* states_delta /*or NULL*/, const float* actions /*or NULL*/,
                             const float* attrs, const int32_t* particle_nums, const float* particle_dens, int B, int N,
                             const float* targets /*[B][H][M][3]*/, const int32_t* target_nums /*[B][H]*/, int M,
                             const double* eps /*[B]*/, int iters, int mode, double* loss_out, float* grad_out,
                             double* col_err_out /*[H][B], nullable*/);

/* ---- Sinkhorn divergence of two padded cloud batches and its gradient: drp_cloud_transport's loss with its
 * entropic bias taken out.  An entropy-regularised plan blurs every particle's mass over its neighbours, so the cloud that
 * minimises the transport term over p is a shrunken copy of q: at p == q the transport gradient is not zero, and descent on it
 * pulls a pile inward.  tests/test_divergence_host.py measures both on the float64 definition (a jittered 0.02 grid, eps = 0.02^2,
 * K = 50): at p == q, 40 points, the transport gradient's largest component is 1.0e-4, a seventh of the 7.1e-4 of two unrelated
 * clouds, where the divergence's is 1.2e-8 and its value -9e-14 against a transport term of 1.1e-4; 200 steps of descent from
 * p = q shrink a 64-point pile's radius of gyration by 4.3 % under transport and move it by 2e-7 of itself under the divergence.
 * The divergence
 *       S(p, q) = OT(p, q) - OT(p, p) / 2 - OT(q, q) / 2     on the dual values
 * is non-negative, zero only for equal clouds, sees density and gives every real row a gradient for any pair of counts.  Per
 * problem (one sample at one rollout step), with n_p and n_q real rows, a = 1/n_p, b = 1/n_q, eps = eps[b] > 0, K = iters:
 *   Cross problem.  Exactly drp_cloud_transport's cost and sweeps: f = 0, then K times g's update and f's.
 *                P_ij = a b exp((f_i + g_j - C_ij)/eps).
 *   Self problem of a cloud x with n rows and mass m = 1/n.  h = 0.  K times, for every j:
 *                h_j <- (h_j + (-eps LSE_i((h_i - C^xx_ij)/eps + log m))) / 2.  Every h_i on the right is the previous sweep's
 *                value (Jacobi form, two arrays).  LSE is max-shifted as in the cross problem.
 *                S_ij = m^2 exp((h_i + h_j - C^xx_ij)/eps) is symmetric by construction.
 *   Value.       divergence = scale (sum_i a f_i + sum_j b g_j - sum_i a h^p_i - sum_j b h^q_j) / 3.  This is the dual form, not
 *                sum P C: the non-negativity holds for it, and the gradient below is its gradient at convergence.  It is not
 *                clamped: rounding or too few sweeps can leave it a hair below zero at p ~ q.
 *   Gradient.    d/dp_i = (2 scale / 3) (sum_j P_ij (p_i - q_j) - sum_j S^p_ij (p_i - p_j)).  P and S are constants of the
 *                derivative.  The differences are fp32 and widened, both sums are in double, and their difference is rounded
 *                once to fp32.  Padding rows get +0.0.  The q-q problem contributes to the value only.
 *   Certificates.  col_err as drp_cloud_transport's.  self_err = [sum_i |sum_j S^p_ij - a|, sum_j |sum_i S^q_ij - b|].  Outputs,
 *                not stopping rules.
 *   Fixed work, non-finite input, determinism.  As drp_cloud_transport: the loops are counted by K, n_p and n_q alone; no
 *                atomics, one summation order; the bits depend on the two counts, not on the padded N and M, on B or on the
 *                neighbouring samples.
 * dual_out [B][2N + 2M]: f, g, h^p, h^q, 0 on padding.  Contract and refusals as drp_cloud_transport (every output but
 * terms_out is nullable); it counts under the "loss" kernel class of drp_probe_begin.  Its float64 yardstick is
 * drp_cloud_divergence_f64 / drp_train_grad_f64_divergence below. */
int drp_cloud_divergence(drp_ctx* ctx, const float* p, const int32_t* n_p, const float* q, const int32_t* n_q,
                         int B, int N, int M, const double* eps /*[B]*/, int iters, double* terms_out /*[B]*/,
                         float* grad_p_out /*[B][N][3], nullable*/, double* dual_out /*[B][2N+2M]: f, g, h_p, h_q, nullable*/,
                         double* col_err_out /*[B], nullable*/, double* self_err_out /*[B][2], nullable*/);

/* drp_train_step_transport with the divergence of drp_cloud_divergence as each step's term: the same arguments, refusals and
 * contract, plus self_err_out [H][B][2] (nullable): every problem's self_err. */
int drp_train_step_divergence(drp_ctx* ctx, const float* states, const float* states_delta /*or NULL*/, const float* actions /*or NULL*/,
                              const float* attrs, const int32_t* particle_nums, const float* particle_dens, int B, int N,
                              const float* targets /*[B][H][M][3]*/, const int32_t* target_nums /*[B][H]*/, int M,
                              const double* eps /*[B]*/, int iters, int mode, double* loss_out, float* grad_out,
                              double* col_err_out /*[H][B], nullable*/, double* self_err_out /*[H][B][2], nullable*/);

/* ---- Unbalanced Sinkhorn divergence (csrc/k_sinkhorn.h: kd_sweeps_unbalanced): drp_cloud_divergence for a pile
 * seen partly.  The balanced plan must place every predicted particle's mass on the observed cloud, so a particle whose
 * counterpart was not observed is pulled hardest.  Here each marginal is held by a KL penalty in place of the hard constraint
 * (Sejourne et al. 2019): mass further than about sqrt(rho) from the other cloud is given up, not moved.  Two more quantities per
 * problem: the reach rho = rho[b] > 0, in squared-distance units like eps, and the target cloud's total mass w = mass_q[b] > 0.
 * a = 1/n_p per predicted row (total 1), b = w/n_q per target row (total w), lambda = rho / (rho + eps).  Notation as above.
 *   Cross problem.  f = 0.  K times: g_j <- lambda (-eps LSE_i((f_i - C_ij)/eps + log a)), then
 *                f_i <- lambda (-eps LSE_j((g_j - C_ij)/eps + log b)).  P_ij = a b exp((f_i + g_j - C_ij)/eps).
 *   Self problem of a cloud with per-row mass m (a for p, b for q).  h = 0.  K times, Jacobi on the previous sweep's h:
 *                h_j <- (h_j + lambda (-eps LSE_i((h_i - C_ij)/eps + log m))) / 2.  S_ij = m^2 exp((h_i + h_j - C_ij)/eps).
 *   Value.       scale (rho + eps/2) [sum_i a (expm1(-h^p_i/rho) - expm1(-f_i/rho)) + sum_j b (expm1(-h^q_j/rho) - expm1(-g_j/rho))] / 3,
 *                not clamped.  At the fixed point this is OT_rho(p,q) - OT_rho(p,p)/2 - OT_rho(q,q)/2 + (eps/2)(1 - w)^2: every
 *                term in the masses cancels.  expm1 because the two exponentials cancel for large rho; the limit for
 *                rho -> inf is the balanced value.  Summed as -expm1(-f/rho) and -expm1(-g/rho) in the cross problem's order, less
 *                the two self problems' sums, times (rho + eps/2).
 *   Gradient.    The balanced expression with these P and S^p: the cost enters the relaxed problem through <P, C> alone.
 *   Certificates.  col_err = sum_j |sum_i P_ij - b exp(-g_j/rho)| (the row identity sum_j P_ij = a exp(-f_i/rho) holds exactly
 *                behind f's update).  self_err = [sum_i |sum_j S^p_ij - a exp(-h^p_i/rho)|, sum_j |sum_i S^q_ij - b exp(-h^q_j/rho)|].
 *                transported = sum_i a exp(-f_i/rho): the plan's total mass, the share of the predicted pile the loss pairs
 *                with something; 1 when balanced.
 *   rho = +inf   is allowed and means lambda = 1, the balanced value and certificates.  It requires w == 1 exactly (balanced
 *                transport between unequal masses has no plan); every output then has drp_cloud_divergence's bits.
 * Refused with DRP_EINVAL and a message, on the host, before any launch: everything drp_cloud_divergence refuses; rho or mass_q
 * NULL; rho[b] not (finite with rho[b] >= eps[b]/1024, or +inf) -- below that f/rho means nothing but "no transport";
 * mass_q[b] outside [1/8, 8]; mass_q[b] != 1 with rho[b] = +inf.  Same grid, LDS and fixed work as drp_cloud_divergence.  The
 * float64 yardstick is drp_cloud_divergence_unbalanced_f64 / drp_train_grad_f64_divergence_unbalanced below. */
int drp_cloud_divergence_unbalanced(drp_ctx* ctx, const float* p, const int32_t* n_p, const float* q, const int32_t* n_q,
                                    int B, int N, int M, const double* eps /*[B]*/, const double* rho /*[B]*/,
                                    const double* mass_q /*[B]*/, int iters, double* terms_out /*[B]*/,
                                    float* grad_p_out /*[B][N][3], nullable*/, double* dual_out /*[B][2N+2M]: f, g, h_p, h_q, nullable*/,
                                    double* col_err_out /*[B], nullable*/, double* self_err_out /*[B][2], nullable*/,
                                    double* transported_out /*[B], nullable*/);

/* drp_train_step_divergence with drp_cloud_divergence_unbalanced as each step's term: rho [B] per sample, mass_q [H][B] per
 * problem (step-major, as the certificates), transported_out [H][B] (nullable).  The same refusals on top of that call's. */
int drp_train_step_divergence_unbalanced(drp_ctx* ctx, const float* states, const float* states_delta /*or NULL*/,
                                         const float* actions /*or NULL*/, const float* attrs, const int32_t* particle_nums,
                                         const float* particle_dens, int B, int N, const float* targets /*[B][H][M][3]*/,
                                         const int32_t* target_nums /*[B][H]*/, int M, const double* eps /*[B]*/,
                                         const double* rho /*[B]*/, const double* mass_q /*[H][B]*/, int iters, int mode,
                                         double* loss_out, float* grad_out, double* col_err_out /*[H][B], nullable*/,
                                         double* self_err_out /*[H][B][2], nullable*/, double* transported_out /*[H][B], nullable*/);

/* ---- the float64 yardstick of the Sinkhorn divergence (csrc/k_sinkhorn.h).  drp_cloud_divergence's definition with nothing
 * in fp32: p is DOUBLE [B][N][3] -- on purpose: the call runs the instantiation the trainer's yardstick runs on the float64
 * tape's predicted state -- q the caller's floats widened exactly; every cost, of p - q, p - p and q - q, is dx*dx + dy*dy + dz*dz
 * in double in that order on double differences (no fused multiply-add); the gradient (2 scale / 3) (sum_j P_ij (p_i - q_j) -
 * sum_j S^p_ij (p_i - p_j)) is written as double with no rounding to fp32, +0.0 on padding; the value is the dual form, not
 * clamped.  Sweeps, (output, part) mapping, summation orders, fixed work and determinism are drp_cloud_divergence's: the bits
 * depend on the two counts alone.  The same one-shot contract: no weights needed, no session ended, every output but terms_out
 * nullable, a refused call leaves the context usable.  Refusals as drp_cloud_divergence, on the host: N or M above 1024 points
 * (DRP_EINVAL), counts outside 1..N / 1..M, eps not positive and finite, iters outside 1..DRP_TRANSPORT_MAX_ITERS, a real row
 * that is not finite.  It is no dispatch variant; like drp_cloud_divergence it counts under the "loss" kernel class of
 * drp_probe_begin (one timed region around its two kernels). */
int drp_cloud_divergence_f64(drp_ctx* ctx, const double* p /*[B][N][3]*/, const int32_t* n_p, const float* q, const int32_t* n_q,
                             int B, int N, int M, const double* eps /*[B]*/, int iters, double* terms_out /*[B]*/,
                             double* grad_p_out /*[B][N][3], nullable*/, double* dual_out /*[B][2N+2M]: f, g, h_p, h_q, nullable*/,
                             double* col_err_out /*[B], nullable*/, double* self_err_out /*[B][2], nullable*/);

/* drp_train_grad_f64_untracked with the Sinkhorn divergence of drp_train_step_divergence in place of the Chamfer loss: the
 * yardstick of drp_train_step_divergence's gradients, row u4.  The term of (step t, sample b) is drp_cloud_divergence_f64's value
 * / (n_rollout B) between the DOUBLE prediction s_pred_t[b, :n_b] and targets[b, t, :target_nums[b, t]] with eps[b] and iters
 * sweeps; it seeds the reverse pass with that call's gradient (the cross plan and the prediction's self plan constants of the
 * derivative) on real rows and +0.0 on padded ones, and everything behind the seed is drp_train_grad_f64's code.  The plans are
 * formed HERE from the double prediction: the fp32 trainer's plans are no input, so the difference of the two gradients includes
 * what the fp32 state's drift does to exp(. / eps).  col_err_out [n_rollout][B] and self_err_out [n_rollout][B][2] (nullable):
 * every problem's certificates.  Exactly one of states_delta and actions; of states only step 0 is read.  The same bits from run
 * to run and under any workspace cap.  The one-shot contract is drp_train_grad_f64's: no drp_train_begin; the Adam state, the
 * selected engine, the dispatch marks and the float64 taps are untouched.  Refusals: those of drp_train_grad_f64_untracked, and
 * DRP_EINVAL for N or M above 1024 and for eps / iters as drp_cloud_transport refuses them.  The matching losses' yardstick is
 * drp_train_grad_f64_match below; the transport loss has none. */
int drp_train_grad_f64_divergence(drp_ctx* ctx, const float* states, const float* states_delta /*[B][H][N][3] or NULL*/,
                                  const float* actions /*[B][H][4] or NULL*/, const float* attrs, const int32_t* particle_nums,
                                  const float* particle_dens, int B, int N, int n_rollout,
                                  const float* targets /*[B][H][M][3]*/, const int32_t* target_nums /*[B][H]*/, int M,
                                  const double* eps /*[B]*/, int iters, double* loss_out, double* loss_terms_out, double* grad_out,
                                  double* grad_state_out, double* col_err_out /*[H][B], nullable*/,
                                  double* self_err_out /*[H][B][2], nullable*/);

/* ---- the float64 yardstick of the unbalanced Sinkhorn divergence (csrc/k_sinkhorn.h: kd64_sweeps_unbalanced,
 * kd64_combine_unbalanced).  drp_cloud_divergence_unbalanced's definition -- sweeps damped by lambda, the clouds' own masses, the
 * expm1 value times (rho + eps/2), the certificates against mass exp(-dual/rho), transported -- with drp_cloud_divergence_f64's
 * arithmetic: p DOUBLE, q widened exactly, double costs on double differences, the gradient written as double, +0.0 on padding.
 * rho [B], mass_q [B], transported_out [B] (nullable).  The contract and the launches are drp_cloud_divergence_f64's (grid, LDS,
 * fixed work, bits a function of the counts alone, the "loss" kernel class); rho[b] = +inf with mass_q[b] = 1 returns
 * drp_cloud_divergence_f64's bits on every output and transported = sum_i a.  Refused on the host, before any launch: everything
 * drp_cloud_divergence_f64 refuses and everything drp_cloud_divergence_unbalanced refuses of rho and mass_q; the context stays
 * usable. */
int drp_cloud_divergence_unbalanced_f64(drp_ctx* ctx, const double* p /*[B][N][3]*/, const int32_t* n_p, const float* q,
                                        const int32_t* n_q, int B, int N, int M, const double* eps /*[B]*/, const double* rho /*[B]*/,
                                        const double* mass_q /*[B]*/, int iters, double* terms_out /*[B]*/,
                                        double* grad_p_out /*[B][N][3], nullable*/,
                                        double* dual_out /*[B][2N+2M]: f, g, h_p, h_q, nullable*/, double* col_err_out /*[B], nullable*/,
                                        double* self_err_out /*[B][2], nullable*/, double* transported_out /*[B], nullable*/);

/* drp_train_grad_f64_divergence with drp_cloud_divergence_unbalanced_f64 as each step's term: the yardstick of
 * drp_train_step_divergence_unbalanced's gradients.  rho [B] per sample, mass_q [n_rollout][B] per problem (step-major, as the
 * certificates), transported_out [n_rollout][B] (nullable).  The three arrays belong to the batch: the bits are the same under
 * any workspace cap.  The same refusals as drp_train_grad_f64_divergence, and rho / mass_q as
 * drp_train_step_divergence_unbalanced refuses them. */
int drp_train_grad_f64_divergence_unbalanced(drp_ctx* ctx, const float* states, const float* states_delta /*[B][H][N][3] or NULL*/,
                                             const float* actions /*[B][H][4] or NULL*/, const float* attrs,
                                             const int32_t* particle_nums, const float* particle_dens, int B, int N, int n_rollout,
                                             const float* targets /*[B][H][M][3]*/, const int32_t* target_nums /*[B][H]*/, int M,
                                             const double* eps /*[B]*/, const double* rho /*[B]*/, const double* mass_q /*[H][B]*/,
                                             int iters, double* loss_out, double* loss_terms_out, double* grad_out,
                                             double* grad_state_out, double* col_err_out /*[H][B], nullable*/,
                                             double* self_err_out /*[H][B][2], nullable*/, double* transported_out /*[H][B], nullable*/);

/* ---- the float64 yardstick of the matching losses (csrc/k_match_f64.h).  drp_cloud_match's definition with nothing in fp32: p
 * is DOUBLE [B][N][3] -- on purpose: the call runs the kernel the trainer's yardstick runs on the float64 tape's predicted state --
 * q the caller's floats widened where they are loaded; C[i][j] = dx*dx + dy*dy + dz*dz in double, in that order, on double
 * differences (no fused multiply-add).  The solver is drp_cloud_match's: shortest augmenting paths with duals, rows of the smaller
 * cloud (p's where the counts are equal) inserted in ascending index, the lowest column index among equal shortest reduced
 * costs; u, v, shortest distances and reduced costs double; no atomics; every loop counted by r and c alone.  One wavefront per
 * problem, column j on lane j & 63 whatever the sizes: the bits depend on the two counts and the values alone, not on N, M, B, the
 * padding or the samples around.
 *   terms_out [B]       sum_pairs |p_i - q_sigma(i)|^2 / (3 r) on double differences, summed in ascending row index of p
 *   grad_p_out          2 (p_i - q_sigma(i)) / (3 r) on matched rows, +0.0 exactly on unmatched rows and padding; double
 *   match_pq_out, match_qp_out   the OPTIMUM's partners, -1 on unmatched rows and padding
 *   dual_out [B][N+M]   the optimum's duals u then v, 0 on padding and on the larger cloud's unmatched rows
 *   cost_out [B][2]     sum C over the pairs the term used, then over the optimum's pairs
 * match_in [B][N] (nullable): a matching given by the caller -- the partner in q of every row of p, -1 for none.  The term and
 * the gradient are then taken on the caller's pairs; the solver runs all the same and its own optimum goes to match_pq_out,
 * match_qp_out, dual_out and cost_out[.][1].  With match_in NULL the two costs are equal; otherwise the first is never below the
 * second.  The one-shot contract of drp_cloud_match: no weights needed, no session ended, the engine, drp_last_dispatch and the
 * trainer left alone; it counts under the "loss" kernel class of drp_probe_begin.
 * DRP_EINVAL (the context stays usable): what drp_cloud_match refuses (a null argument -- every output but terms_out is nullable
 * --, a count outside 1..N or 1..M, N or M outside 1..1024, a real row of p or q that is not finite), and a match_in that is no
 * one-to-one matching of exactly r = min(n_p, n_q) real rows into 0..n_q-1 or has a partner on a padded row (the message names
 * sample, step and row). */
int drp_cloud_match_f64(drp_ctx* ctx, const double* p /*[B][N][3]*/, const int32_t* n_p, const float* q, const int32_t* n_q,
                        int B, int N, int M, const int32_t* match_in /*[B][N], nullable*/, double* terms_out /*[B]*/,
                        double* grad_p_out /*[B][N][3], nullable*/, int32_t* match_pq_out /*[B][N], nullable*/,
                        int32_t* match_qp_out /*[B][M], nullable*/, double* dual_out /*[B][N+M], nullable*/,
                        double* cost_out /*[B][2], nullable*/);

/* drp_train_grad_f64_untracked with a matching loss of drp_train_step_loss in place of the Chamfer loss: the yardstick of that
 * call's gradients for loss_kind DRP_LOSS_MATCH and DRP_LOSS_CHAMFER_MATCH (another kind: DRP_EINVAL), row u2.  The term of
 * (step t, sample b) is drp_cloud_match_f64's / (n_rollout B) between the DOUBLE prediction s_pred_t[b, :n_b] and
 * targets[b, t, :target_nums[b, t]]; it seeds the reverse pass with that call's gradient, and everything behind the seed is
 * drp_train_grad_f64's code.  The mix: the float64 Chamfer kernel runs first and leaves a Chamfer-only step's terms and seed, the
 * matching kernel behind it in the stream turns each element into (1 - w) x it + w x its own share, in double -- one writer
 * per element, stream order, drp_train_step_loss's scheme.
 * match_in [n_rollout][B][N] (nullable; drp_train_step_loss's match_out layout): the pairs of every term and seed, as
 * drp_cloud_match_f64's match_in.  With the fp32 trainer's partners given here, the difference of the two calls' gradients is
 * arithmetic error on the SAME pairs -- a partner that the fp32 tape's drift of about 1e-6 of a spacing flipped is no part of it.
 * The assignment is solved in double all the same: match_out [n_rollout][B][N] (nullable) is the float64 side's own optimum,
 * cost_out [n_rollout][B][2] (nullable) sum C over the pairs used, then over the optimum's -- equal with match_in NULL, the first
 * never below the second otherwise --, margin_out [n_rollout][B] (nullable; written for the mix only) the Chamfer arg-min margins
 * of drp_train_grad_f64_untracked.  Exactly one of states_delta and actions; of states only step 0 is read.  The same bits from
 * run to run and under any workspace cap.  The one-shot contract of drp_train_grad_f64_untracked.  Refusals (DRP_EINVAL, the
 * context stays usable): those of drp_train_grad_f64_untracked and of drp_train_step_loss -- N or M above 1024, match_weight
 * outside (0, 1) for the mix (it is read by the mix only) --, another loss_kind, and a match_in as drp_cloud_match_f64 refuses it.
 * The transport loss has no float64 yardstick. */
int drp_train_grad_f64_match(drp_ctx* ctx, const float* states, const float* states_delta /*[B][H][N][3] or NULL*/,
                             const float* actions /*[B][H][4] or NULL*/, const float* attrs, const int32_t* particle_nums,
                             const float* particle_dens, int B, int N, int n_rollout,
                             const float* targets /*[B][H][M][3]*/, const int32_t* target_nums /*[B][H]*/, int M, int loss_kind,
                             double match_weight, const int32_t* match_in /*[H][B][N], nullable*/, double* loss_out,
                             double* loss_terms_out, double* grad_out, double* grad_state_out,
                             int32_t* match_out /*[H][B][N], nullable*/, double* cost_out /*[H][B][2], nullable*/,
                             double* margin_out /*[H][B], nullable*/);

/* ---- training on a loss of the CALLER's: every step's prediction out, d loss / d s_pred in -------------------------------------
 * In drp_train_step every loss kernel does three things: it writes d loss / d s_pred_t of every step, the loss terms, and it
 * zero-fills the gradient blob.  These two calls open that seam, statelessly: the first returns what the training forward
 * predicts, the second runs the same forward again and seeds the reverse pass with an array of the caller's.  The forward is
 * deterministic, so the second call's predictions are the bits the first returned and the seed is the gradient at the right
 * point; the price is one forward more per update.  The batch arguments and their refusals are drp_train_step_loss's: exactly one
 * of states_delta and actions, actions needs a camera and refuses a push of zero length.
 *
 * drp_train_predict: the forward EXACTLY as drp_train_step_seeded (and drp_train_step with DRP_TRAIN_GRAD) runs it -- the tape
 * engine of the same selection, the tape written, zero-padded rows joining the graph -- and states_pred_out [B][n_rollout][N][3]:
 * on rows n < particle_nums[b] the bits of that call's own forward.  (The DRP_TRAIN_EVAL forward runs without the tape and is
 * promised nothing here.)  Rows n >= particle_nums[b] come back as the forward leaves them and are no part of the contract.
 * Needs drp_train_begin (n_rollout is its); changes no weight, no Adam moment and no iteration count.
 *
 * drp_train_step_seeded: seed [B][n_rollout][N][3], seed[b, t, n, :] = d loss / d s_pred_t[b, n], COMPLETE -- the library applies
 * no 1 / (n_rollout B) and no 1 / (3 n_b).  Rows n >= particle_nums[b] of the seed are never read as numbers: the reverse pass
 * sees +0.0 there whatever they hold.  Everything behind the seed -- the reverse pass, the push's position share with actions, the
 * weight gradients, Adam, re-packing, the one wait -- is drp_train_step's own code; fed drp_train_step's own seed, 2 (s_pred -
 * s_nxt) / (3 n_b n_rollout B) formed with its fp32 operations from drp_train_predict's output, grad_out has the bits of
 * drp_train_step's.  mode DRP_TRAIN_GRAD or DRP_TRAIN_UPDATE.  There is no loss argument: the value is the caller's.  No dispatch
 * variant of its own.  Refusals: DRP_ESTATE without drp_train_begin (or, with actions, without a camera); DRP_EINVAL for a null
 * argument, both or neither impulse source, a count outside 1..N, a value on a real row of the seed that is infinite or no number
 * (the message names sample, step and row), DRP_TRAIN_EVAL (the forward alone is drp_train_predict).  A refused call leaves the
 * context as it was. */
int drp_train_predict(drp_ctx* ctx, const float* states, const float* states_delta /*[B][H][N][3] or NULL*/,
                      const float* actions /*[B][H][4] or NULL*/, const float* attrs, const int32_t* particle_nums,
                      const float* particle_dens, int B, int N, float* states_pred_out /*[B][H][N][3]*/);
int drp_train_step_seeded(drp_ctx* ctx, const float* states, const float* states_delta /*[B][H][N][3] or NULL*/,
                          const float* actions /*[B][H][4] or NULL*/, const float* attrs, const int32_t* particle_nums,
                          const float* particle_dens, int B, int N, const float* seed /*[B][H][N][3]*/, int mode,
                          float* grad_out /*nullable*/);
/* The same pair in float64, on drp_train_grad_f64's tape and reverse pass: the yardstick of the two calls above.  The forward of
 * both is drp_train_grad_f64's; states_pred_out and seed are doubles [B][n_rollout][N][3]; grad_out [38 403] (nullable) and
 * grad_state_out [B][n_rollout][N][3] (nullable) as drp_train_grad_f64's.  The seed is sliced per chunk of samples; the outputs are
 * the same bits from run to run and under any workspace cap.  The one-shot contract of drp_train_grad_f64: no drp_train_begin
 * needed, buffers of their own, the engine, the sessions, the Adam state, the dispatch marks and the float64 taps untouched.
 * Refusals (DRP_EINVAL): those of drp_train_grad_f64_untracked's batch arguments, a null seed or output, a value on a real row of
 * the seed that is infinite or no number. */
int drp_train_predict_f64(drp_ctx* ctx, const float* states, const float* states_delta /*[B][H][N][3] or NULL*/,
                          const float* actions /*[B][H][4] or NULL*/, const float* attrs, const int32_t* particle_nums,
                          const float* particle_dens, int B, int N, int n_rollout, double* states_pred_out /*[B][H][N][3]*/);
int drp_train_grad_f64_seeded(drp_ctx* ctx, const float* states, const float* states_delta /*[B][H][N][3] or NULL*/,
                              const float* actions /*[B][H][4] or NULL*/, const float* attrs, const int32_t* particle_nums,
                              const float* particle_dens, int B, int N, int n_rollout, const double* seed /*[B][H][N][3]*/,
                              double* grad_out, double* grad_state_out);

/* ---- the optimiser seam: accumulate gradients, clip by global norm, keep Adam's state -----------------------------------------
 * Every drp_train_step* entry point ends in the same optimiser: one Adam step on that one call's gradient.  With mode
 * DRP_TRAIN_GRAD each of them leaves its gradient on the device and the weights untouched; these four calls are what comes behind
 * it, once for all of them.  They change no existing call.  The context keeps a "fresh gradient" mark: a DRP_TRAIN_GRAD pass of
 * any entry point that returns DRP_OK sets it; drp_train_accumulate clears it, and so does everything that writes the gradient
 * buffer or ends training -- every drp_train_step* call in any mode (refused ones included), drp_train_predict, drp_train_begin,
 * drp_train_apply and drp_load_weights.
 *
 * drp_train_accumulate: acc[i] += weight * (double)grad[i] over the 38 403 entries of a float64 accumulator on the device, which
 * drp_train_begin allocates and zeroes; grad is the last pass's gradient where it lies (no host copy, no wait).  A pass can be
 * accumulated once.  An integer weight up to 2^29 times an fp32 value is exact in double (24 + 29 bits), so an accumulator fed
 * sample counts is the exact sum of the weighted gradients in call order, rounded once per addition -- what the trainer uses
 * (weight = B, then scale = 1 / sum B).  DRP_ESTATE without drp_train_begin or without a fresh gradient; DRP_EINVAL for a weight
 * that is not finite or not > 0.
 *
 * drp_train_apply: s0 = scale; norm = || s0 acc ||_2 in double, reduced in a fixed order without atomics (the same bits from run
 * to run); clip = min(1, max_norm / (norm + 1e-6)), torch's clip_grad_norm_ (max_norm = +inf: no clipping, clip = 1); s = s0 *
 * clip, one double product; g32[i] = (float)(acc[i] * s); one Adam step on g32 with drp_train_step's arithmetic and bias
 * corrections; the device re-pack of drp_train_step; the accumulator zeroed and the iteration count advanced.  One host wait; the
 * norm does not come to the host between the reduction and the Adam launch.  With weight 1, scale 1 and no clipping the weights,
 * Adam's moments and the iteration count have the bits DRP_TRAIN_UPDATE leaves on the same batch.  A norm that is not finite
 * (decided on the device) moves nothing: weights, moments, iteration count and packed copies keep their bits, the accumulator is
 * still cleared, *applied_out = 0 and the call returns DRP_OK.  A step that is applied ends the planner sessions, as every update
 * does; a skipped one ends none.  norm_out, clip_out, applied_out and grad_out [38 403] (g32, in
 * drp_get_weights' layout) are nullable.  DRP_ESTATE without drp_train_begin or with nothing accumulated since the last
 * drp_train_apply / drp_train_begin; DRP_EINVAL for a scale that is not finite or not > 0 and for max_norm NaN or <= 0.  A
 * refused call leaves the context as it was.
 *
 * drp_train_get_state / drp_train_set_state: Adam's m and v (38 403 floats each, drp_get_weights' layout) and the number of
 * steps taken, so that a resumed run continues with the bits of an uninterrupted one.  The accumulator is no part of the state.
 * Both need drp_train_begin (DRP_ESTATE); set_state refuses a value that is not finite, a negative v and a negative iter with
 * DRP_EINVAL and then changes nothing. */
int drp_train_accumulate(drp_ctx* ctx, double weight);
int drp_train_apply(drp_ctx* ctx, double scale, double max_norm /* +inf: no clipping */, double* norm_out, double* clip_out,
                    int* applied_out, float* grad_out /* nullable, 38 403 */);
int drp_train_get_state(drp_ctx* ctx, float* m_out, float* v_out, int64_t* iter_out);
int drp_train_set_state(drp_ctx* ctx, const float* m, const float* v, int64_t iter);

#ifdef __cplusplus
}
#endif
#endif /* DRP_H */
