/*
 * merlin_hip.h -- C ABI of libmerlin_hip.so, the MI355X (gfx950) hot path of
 * PPO-2DGrid ("MERLIN"): batched MiniGrid step/reset dynamics, the occluded
 * 7x7 egocentric observation, reward/done rules, the RGB tile expansion, and
 * GAE(lambda) + advantage normalisation.
 *
 * Conventions
 *   - Plain C types only; every device pointer is caller-allocated (e.g. a
 *     torch tensor's data_ptr()) and every call is stream-ordered on `stream`
 *     (a hipStream_t passed as void*; NULL = the null stream).  Calls marked
 *     [sync] synchronise that stream.
 *   - The env context owns only per-env state (grid bitmasks, agent, RNG,
 *     episode accumulators) in device memory.
 *   - Every entry point returns 0 (MERLIN_OK) or a MERLIN_E* code; nothing
 *     throws across the ABI.  merlin_last_error() gives a thread-local message.
 *   - Not re-entrant per context; one host thread per device.
 *
 * Reference interfaces replaced (paths relative to the reference checkout):
 *   merlin_env_create    gym.make(env_id, size=..) + wrapper chain
 *                        src/scenario_creator/scenario_creator.py:35-57,
 *                        BaseCustomEnv.__init__ src/custom_envs/base_env.py:15-41
 *   merlin_env_seed      gymnasium Env.reset(seed=s) -> seeding.np_random(s)
 *                        (ppo/ppo_train.py:48 `env.reset(seed=base_seed + ep)`)
 *   merlin_env_reset     env.reset() src/ppo.py:35,65,96 -> MiniGridEnv.reset ->
 *                        <Difficulty>Env._gen_grid (medium_hard_env.py:12-45,
 *                        hard_env.py:11-73, easy/medium/hardest_env.py)
 *   merlin_env_step      env.step(action.item()) src/ppo.py:76 ->
 *                        ThreeActionWrapper.action (three_action_wrapper.py:16-17)
 *                        -> MiniGridEnv.step [+ StuckPenaltyWrapper.step
 *                        stuck_penalty_wrapper.py:29-57]; done = term or trunc
 *                        (src/ppo.py:77); auto-reset on done (src/ppo.py:93-98)
 *   obs codes            RGBImgPartialObsWrapper.observation -> get_pov_render
 *                        (gen_obs_grid + process_vis), selected at
 *                        scenario_creator.py:48
 *   merlin_obs_expand_*  Grid.render tile blit + ImgObsWrapper
 *                        (scenario_creator.py:50), PPO._obs_to_tensor
 *                        src/ppo.py:58-62, CNNActorCritic._format_obs
 *                        src/actor_critic.py:43-46 and the /255 of
 *                        CNNFeatureExtractor.forward src/actor_critic.py:20-21
 *   merlin_gae           PPO.compute_gae src/ppo.py:107-120
 *                        (== compute_gae_standard src/utils/utils_rl.py:11-29)
 *   merlin_adv_normalize (adv - adv.mean()) / (adv.std() + 1e-8) src/ppo.py:125
 *   merlin_conv1_lut_*   the first Conv2d(3,32,k8,s4)+ReLU of both CNNFeatureExtractor
 *                        towers (src/actor_critic.py:9-10,20-21) evaluated from the
 *                        tile codes, and its weight/bias gradient
 *   merlin_tower_*       the data-movement stages around the conv2/conv3 GEMMs of the
 *                        towers (actor_critic.py:11-14): conv1 -> conv2 im2col from codes,
 *                        conv2 bias+ReLU -> conv3 im2col, and their backward passes;
 *                        merlin_tower_conv2_lut_*: Conv2d(3,32,k8,s4)+ReLU+Conv2d(32,64,k4,s2)
 *                        of both towers (actor_critic.py:9-12) as table lookups from the
 *                        tile codes, and the table gradient
 *   merlin_tower_window_*, merlin_segment_sum: the same conv2 and the following
 *                        Conv2d(64,64,k3,s1)+ReLU (actor_critic.py:13-14) evaluated once per
 *                        distinct receptive-field window of an update, and the fixed-order
 *                        segmented sums of their backward pass (merlin/windows.py)
 *   merlin_tower_bias_relu / _relu_bwd / _head_bwd: the ReLU + bias epilogues of the
 *                        conv3 / fc1 GEMMs and the heads' backward (actor_critic.py:14-41)
 *
 * What the benched loop (bench.py, BASELINE cfg 2) calls, per rollout step: merlin_tower_codes_conv3_amax,
 * merlin_h3_gemm_nt_heads (cfg 12, heads only), merlin_env_act_step; per rollout: merlin_env_refill (the ring of
 * look-ahead maps topped up once, merlin_env_set_lookahead_depth); per update:
 * merlin_gae, merlin_adv_normalize, merlin_minibatch_patch_maps, and per optimizer step merlin_window_lut_*,
 * merlin_window_gemm_fwd / _bwd, merlin_tower_window_conv3_planes, merlin_h3_gemm_nt_heads (cfg 60),
 * merlin_ppo_loss*, merlin_tower_head_bwd_planes, merlin_h3_gemm_nt_planes (cfg 62),
 * merlin_h3_gemm_tn_gather_planes_a (cfg 20), merlin_segment_sum_* (R / S / dQ / dT2), merlin_stage_*,
 * merlin_clip_adam.  The rest serve the other drop-in paths -- the gym single env and the frame path (obs
 * expansion, conv1 / conv2 lookups per frame, im2col), the autograd window path, FOMAML (merlin_group_act), few-shot
 * evaluation (merlin_group_clip_sgd, merlin_episode_loss: src/distribution_over_tasks.py:97-128, :200-203) -- or
 * are ALTERNATE forms kept selectable for A/B and float64 precision tests: merlin_x6_* (fc1 in six bf16
 * products, rounds 2-3), merlin_h3_gemm_nt / _tn / _tn_planes / _nt_gather with the register-staged
 * configurations (round 4).
 */
#ifndef MERLIN_HIP_H
#define MERLIN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MERLIN_ABI_VERSION 3  /* 3: compact acting-table keys (round 5), plane-operand GEMMs */

#define MERLIN_OK 0
#define MERLIN_E_INVALID 1     /* bad argument / config */
#define MERLIN_E_HIP 2         /* a HIP runtime call failed */
#define MERLIN_E_DEVICE 3      /* device-side error flag raised (see merlin_env_errors) */
#define MERLIN_E_UNSUPPORTED 4 /* e.g. grid size outside 5..32, hardest below size 8 */

/* difficulty ids (ScenarioCreator difficulties, src/config/scenario.yaml) */
#define MERLIN_EASY 0
#define MERLIN_MEDIUM 1
#define MERLIN_MEDIUMHARD 2
#define MERLIN_HARD 3
#define MERLIN_HARDEST 4

/* device error bits reported by merlin_env_errors */
#define MERLIN_DEVERR_BAD_ACTION 1u  /* action not in {0,1,2}: ThreeActionWrapper IndexError */
#define MERLIN_DEVERR_PLACE_OBJ 2u   /* place_obj max_tries exceeded: RecursionError */
#define MERLIN_DEVERR_SLOT_EMPTY 8u  /* a reset met an empty look-ahead slot with the step fallback off */
#define MERLIN_DEVERR_BAD_TILE 4u    /* merlin_tower_codes_conv3: a frame that is no observation (the agent tile (class
                                      * 4) missing at view cell (3, 6) or present elsewhere): merlin_tower_errors */
#define MERLIN_DEVERR_BAD_FRAME 16u  /* a rendered frame's agent was outside the grid, on a wall or had a direction
                                      * outside 0..3, or its env id was out of range: the frame is drawn without the
                                      * agent and its highlight.  merlin_env_render: merlin_env_errors;
                                      * merlin_render_frames: merlin_tower_errors.  merlin_view_codes raises it there
                                      * too, for a pose that has no view */

/* observation layouts for merlin_obs_expand_f32 */
#define MERLIN_LAYOUT_NCHW 0 /* [n][3][56][56]: what CNNActorCritic._format_obs hands the convs */
#define MERLIN_LAYOUT_NHWC 1 /* [n][56][56][3]: the RolloutBuffer / gym observation layout */

/* Observation codes: one 7x7 view per env = 49 tile classes (0 dark-empty,
 * 1 lit empty, 2 lit wall, 3 lit goal, 4 agent), 4 bits each, cell (vi,vj)
 * at nibble vj*7+vi, packed into MERLIN_OBS_WORDS uint32 words (32 B). */
#define MERLIN_OBS_WORDS 8
#define MERLIN_OBS_TILES 5
#define MERLIN_TILE_PX 8
#define MERLIN_VIEW 7

typedef struct merlin_env merlin_env;

typedef struct {
    int32_t num_envs;          /* envs in this context (this rank's shard) */
    int32_t size;              /* grid side, 5..32 (reference: 16, base_env.py:17); hardest: 8..32, the sizes at
                                  which the reference's generator runs (hardest_env.py draws integers(2, size/2 - 1)) */
    int32_t difficulty;        /* MERLIN_* difficulty id */
    int32_t max_steps;         /* <= 0: 4*size^2 (base_env.py:32-33) */
    int32_t stuck_penalty;     /* 1: StuckPenaltyWrapper semantics (off in the reference chain) */
    int32_t max_stay;          /* StuckPenaltyWrapper.max_stay (default 3) */
    double penalty;            /* StuckPenaltyWrapper.penalty (default -0.1) */
    int32_t exploration_bonus; /* 1: +bonus on the first visit of a cell per episode */
    double bonus;
    int32_t reseed_each_reset; /* 1: every reset regenerates from the seeded RNG state, i.e.
                                  env.reset(seed=task_seed) on every episode as FOMAML's
                                  collect_trajectory does (src/fomaml.py:63,92) */
} merlin_env_config;

/* [host] Layout check for bindings that restate merlin_env_config (ctypes, cgo, ...): returns
 * sizeof(merlin_env_config) and writes the byte offset of its first min(n_fields,
 * MERLIN_ENV_CONFIG_FIELDS) fields, in declaration order, to offsets_host (nullable).
 * merlin_env_create reads all MERLIN_ENV_CONFIG_FIELDS fields: a binding must match. */
#define MERLIN_ENV_CONFIG_FIELDS 10
int64_t merlin_env_config_layout(int64_t *offsets_host, int32_t n_fields);

/* Library */
int merlin_version(void);
const char *merlin_last_error(void);
/* [host] the 5 tiles (uint8[5][8][8][3]) the library renders with, computed at
 * load time by the library's own restatement of minigrid's render_tile. */
int merlin_tile_atlas(uint8_t *out_host);

/* Env context */
int merlin_env_create(const merlin_env_config *cfg, merlin_env **out);
int merlin_env_destroy(merlin_env *env);
/* Seed env i with seeds_host[i] (numpy SeedSequence -> PCG64, as gymnasium
 * reset(seed=...)); takes effect at the next merlin_env_reset of that env. */
int merlin_env_seed(merlin_env *env, const uint64_t *seeds_host, int32_t n, void *stream);
/* Give env i the generator diff_host[i] (MERLIN_* ids); NULL restores the context's uniform difficulty.
 * Takes effect at each env's next map generation: every look-ahead slot is invalidated, as merlin_env_seed does
 * (the envs keep their current maps and RNG streams).  n != num_envs or an unknown id: MERLIN_E_INVALID;
 * MERLIN_HARDEST on a context of size < 8: MERLIN_E_UNSUPPORTED, as merlin_env_create.  Stages from host memory
 * and synchronises `stream` before returning.  The classes live in one device buffer allocated with the context,
 * so launches captured into a HIP graph after the first assignment read later assignments without a re-capture;
 * a capture made while the context was uniform (no buffer bound) does not.
 * One lane generates one env's map, so a wave that holds several classes runs their generators one after
 * another.  Every assignment is correct; assignments made of contiguous runs whose boundaries fall on multiples
 * of 64 envs keep every wave of the full-width reset and refill passes on a single generator. */
int merlin_env_set_difficulties(merlin_env *env, const int32_t *diff_host, int32_t n, void *stream);
/* Reset the envs whose mask_dev[i] != 0 (mask_dev NULL = all), writing their
 * observation codes to obs_dev[i][8]; others' obs rows are left untouched. */
int merlin_env_reset(merlin_env *env, const uint8_t *mask_dev, uint32_t *obs_dev, void *stream);
/* Advance all envs n_steps times.  Step t reads actions_dev[t*action_stride + i]
 * (int64, values 0 left / 1 right / 2 forward) and writes, at row t*num_envs+i:
 *   obs_dev[..][8]  observation after the step (after the auto-reset if done),
 *   reward_dev f32, terminated_dev u8, truncated_dev u8, done_dev f32 (term|trunc),
 *   ep_return_dev f64 / ep_length_dev i32 (the finished episode's totals; valid
 *   where done).  Any output pointer may be NULL.  autoreset=0 leaves a done env
 *   in its terminal state (gym semantics: the caller must reset it). */
int merlin_env_step(merlin_env *env, const int64_t *actions_dev, int32_t n_steps,
                    int64_t action_stride, uint32_t *obs_dev, float *reward_dev,
                    uint8_t *terminated_dev, uint8_t *truncated_dev, float *done_dev,
                    double *ep_return_dev, int32_t *ep_length_dev, int32_t autoreset,
                    void *stream);
/* The rollout's act -> env.step in one launch (src/ppo.py:73-76: ac.act(state) then env.step(action.item())):
 * the action of env i is drawn from the acting GEMM's head partials head_part float[2][n_parts][N][4] exactly as
 * merlin_act_draw draws it (log-softmax, argmax or the counter-keyed race keyed by seed, *epoch, step and
 * env_offset + i; biases added; action / logp / value written to action / logp / value, int64 / float / float[N]),
 * then stepped as merlin_env_step with n_steps = 1 and auto-reset.  Output pointers other than action / logp /
 * value may be NULL. */
int merlin_env_act_step(merlin_env *env, const float *head_part_dev, int32_t n_parts, const float *b_actor_dev,
                        const float *b_critic_dev, int32_t act_dim, int32_t deterministic, uint64_t seed,
                        const int64_t *epoch_dev, int64_t step, int64_t env_offset, int64_t *action_dev,
                        float *logp_dev, float *value_dev, uint32_t *obs_dev, float *reward_dev,
                        uint8_t *terminated_dev, uint8_t *truncated_dev, float *done_dev, double *ep_return_dev,
                        int32_t *ep_length_dev, void *stream);
/* FOMAML's acting step (src/fomaml.py:54-108: each task's fast_policy.act(state), src/actor_critic.py:48-56), one
 * frame per task g < groups, each task with its own weights (merlin/grouped_policy.py pack: towers 2g = actor,
 * 2g + 1 = critic): codes_dev int32[groups][8]; T2 float[2G][2720][64] + b2 [2G][64] (conv1 + conv2 tables);
 * W3t [2G][576][64] ((ky, kx, ci) x co) + b3 [2G][64]; W4p [2G][512][576] (fc1, columns (p3, co)) + b4 [2G][512];
 * Wa [G][act_dim][512] + ba [G][act_dim], Wc [G][512] + bc [G] (the heads).  Writes a3_ws [2G][576] (conv3's
 * output) and head_part float[2][8][G][4]: tower t, fc1 column chunk p (64 columns), the chunk's dot products of
 * relu(fc1) with the task's head weights (the biases added in chunk 0) -- the partials merlin_env_act_step reads
 * (with zero biases) to draw and step every task's env.  fp32.  shared_weights = 1: every task acts with ONE weight set
 * (the tensors hold one task's: T2 [2][2720][64], ..., Wa [1][act_dim][512]) -- the support rollout, where every fast
 * policy is still the meta policy (src/fomaml.py:164-171), reads 2 towers' weights instead of 2G copies. */
int merlin_group_act(const uint32_t *codes_dev, int32_t groups, const float *T2_dev, const float *b2_dev,
                     const float *W3t_dev, const float *b3_dev, const float *W4p_dev, const float *b4_dev,
                     const float *Wa_dev, const float *ba_dev, const float *Wc_dev, const float *bc_dev,
                     int32_t act_dim, float *a3_ws_dev, float *head_part_dev, int32_t shared_weights, void *stream);
/* Look-ahead maps (no reference counterpart: an implementation detail of the auto-reset above).
 * An env's next map depends only on its RNG stream, so it is generated ahead of time into a
 * per-env slot, and an auto-reset takes the slot instead of generating in the step.
 * merlin_env_reset refills every slot before it returns; merlin_env_step refills the used slots
 * every `every` step calls (default 16).  every = 0 hands the refills to the caller:
 * merlin_env_refill launches one on `stream` -- e.g. on a side stream after each step, joined
 * before the next step, so the (latency-bound) map generation overlaps the policy forward.  A
 * reset whose slot is empty generates its map in the step instead; results are identical
 * either way. */
int merlin_env_set_refill_interval(merlin_env *env, int32_t every);
int merlin_env_refill(merlin_env *env, void *stream);
/* step_fallback (default on): with refill interval 0, single-step launches are followed by the fallback pass that
 * generates the map of a reset whose slot was empty.  A caller that refills every used slot after EVERY step, before
 * the next one (PPO's rollout: merlin_env_refill on a side stream, joined), can never meet an empty slot and may turn
 * the pass off (one launch -- one graph node -- fewer per step); an empty slot then raises MERLIN_DEVERR_SLOT_EMPTY
 * (merlin_env_errors) and that step's results are invalid. */
int merlin_env_set_step_fallback(merlin_env *env, int32_t on);
/* The look-ahead slot is the head of a ring of `depth` maps per env (default 1: the single slot above, same layout).
 * Slot j holds the env's j-th next map and the RNG state after generating it; slot j + 1 is generated from that
 * state, an auto-reset or merlin_env_reset takes the oldest map, so results are the same at every depth.
 * merlin_env_refill tops every ring up until it is full; a reset that meets an empty ring behaves as one that meets
 * an empty slot.  At depth > 1 with refill interval 0, merlin_env_reset is not followed by a refill: the caller tops
 * up.  A ring that is full when a caller starts serves `depth` resets per env with no refill in between -- a rollout
 * of T steps with the reset at its top uses at most T + 1 (PPO: depth T + 1, one top-up between rollouts, step
 * fallback off).  Nothing may top up a ring while a step or reset of the same env may run.
 * [sync] depth in [1, 65535]; reallocates the ring (num_envs * depth * (4 * SP + 40) bytes, SP = 16 up to size 16,
 * else 32) and drops every look-ahead map; synchronises the device, so it is valid only outside a stream capture,
 * and launches captured before it must be captured again. */
int merlin_env_set_lookahead_depth(merlin_env *env, int32_t depth);
/* The fully observable observation (FullyObsWrapper + ImgObsWrapper, src/scenario_creator/scenario_creator.py:45-50,
 * observation.fully_observable in src/config/scenario.yaml) of every env's current state: out_dev uint8[N][size][size]
 * [3], out[i][x][y] = minigrid Grid.encode's (object, color, state) of cell (x, y), the agent's cell (10, 0, dir).
 * observation.flatten (FlattenObservation, :52-53) is the same bytes read as uint8[N][size*size*3]. */
int merlin_env_full_obs(merlin_env *env, uint8_t *out_dev, void *stream);
/* [sync] copy env state to host: walls uint32[N][size] (bit x of row y = wall at
 * (x,y)); agent int32[N][8] = (x, y, dir, step_count, goal_x, goal_y, stay, 0);
 * rng uint64[N][5] = (state_hi, state_lo, inc_hi, inc_lo, has32<<32|buf32).
 * Any pointer may be NULL. */
int merlin_env_get_state(merlin_env *env, uint32_t *walls_host, int32_t *agent_host,
                         uint64_t *rng_host, void *stream);
/* Full-grid RGB frames: minigrid's render() in rgb_array mode, get_frame(highlight, tile_size) -- the whole grid at
 * tile_size-pixel tiles (4..32; minigrid's default 32), tile (i, j) at img[ts*j : ts*j+ts, ts*i : ts*i+ts], the agent's
 * triangle in its world direction, every cell the agent's 7x7 view shows brightened when highlight != 0.
 * The frame atlas holds the MERLIN_FRAME_TILES = 22 tiles a frame is made of, per tile size, in this order:
 *   0..5    object + 3 * highlighted, object 0 empty / 1 wall / 2 goal, no agent
 *   6..21   6 + ((on_goal * 4 + agent_dir) * 2 + highlighted): the agent on an empty cell (on_goal 0) or on the goal
 *           (1: the terminal state when the caller does not auto-reset), agent_dir 0..3
 * built on first use by the library's restatement of minigrid's render_tile and cached, on the host and per device
 * (the first render of a tile size on a device uploads it: not capturable; later ones are). */
#define MERLIN_FRAME_TILES 22
/* [host] out_host uint8[22][tile_size][tile_size][3]; tile_size outside 4..32: MERLIN_E_INVALID */
int merlin_frame_atlas(int32_t tile_size, uint8_t *out_host);
/* Stateless: frame f < n_frames shows map m = map_index_dev[f] (NULL: f) -- walls_dev uint32[M][size] bit rows as
 * merlin_env_get_state defines them, goal_dev int32[M][2] = (x, y) (NULL or a position outside the grid: no goal) --
 * with the agent agent_dev[f] int32[4] = (x, y, dir, 0).  out_dev uint8[n_frames][size*ts][size*ts][3]; any
 * alignment.  size outside 5..32, tile_size outside 4..32, negative n_frames or a null pointer: MERLIN_E_INVALID.
 * An agent outside the grid, on a wall or with dir outside 0..3 indexes nothing: its frame is drawn without the
 * agent and MERLIN_DEVERR_BAD_FRAME is raised (merlin_tower_errors).  map_index_dev's values are the caller's to
 * keep inside [0, M): the entry is not told M. */
int merlin_render_frames(const uint32_t *walls_dev, const int32_t *goal_dev, const int32_t *agent_dev,
                         const int32_t *map_index_dev, int64_t n_frames, int32_t size, int32_t tile_size,
                         int32_t highlight, uint8_t *out_dev, void *stream);
/* The same kernel on the context's own current state: frame k < n shows env index_dev[k] (int64 env ids; NULL:
 * env k, and n must be num_envs).  An env id outside [0, num_envs): MERLIN_DEVERR_BAD_FRAME (merlin_env_errors). */
int merlin_env_render(merlin_env *env, const int64_t *index_dev, int64_t n, int32_t tile_size,
                      int32_t highlight, uint8_t *out_dev, void *stream);
/* Device-to-device copy of the current state in merlin_render_frames' layouts: walls_dev uint32[N][size], goal_dev
 * int32[N][2], agent_dev int32[N][4].  Any pointer may be NULL.  One kernel, no host sync: capturable. */
int merlin_env_snapshot(merlin_env *env, uint32_t *walls_dev, int32_t *goal_dev, int32_t *agent_dev,
                        void *stream);
/* Shortest action paths (no reference counterpart).  With the step rule of merlin_env_step -- 0 turn
 * left, 1 turn right, 2 forward into a non-wall cell, terminating on the forward action whose front cell is the
 * goal -- dist(x, y, dir) is the least number of actions after which an episode started in that pose terminates, -1
 * if none does.  The goal cell is an ordinary cell for a pose standing on it (dist 4 or 5 there, never 0).
 * Stateless, in merlin_render_frames' layouts: query q < n uses map m = map_index_dev[q] (NULL: q) -- walls_dev
 * uint32[M][size], goal_dev int32[M][2] (a position outside the grid: -1 everywhere) -- and the pose agent_dev[q]
 * int32[4] = (x, y, dir, 0).  dist_dev int32[n]: dist at the query's pose, -1 as well for a pose outside the grid,
 * on a wall or with dir outside 0..3.  field_dev (nullable) int16[n][4][size][size], indexed [dir][y][x]: dist of
 * every pose of the query's map, -1 for walls and unreachable poses; any alignment.  size outside 5..32, negative n
 * or a null required pointer: MERLIN_E_INVALID; n = 0 is a no-op.  map_index_dev's values are the caller's to keep
 * inside [0, M).  One kernel, no allocation, no host sync: capturable. */
int merlin_shortest_paths(const uint32_t *walls_dev, const int32_t *goal_dev, const int32_t *agent_dev,
                          const int32_t *map_index_dev, int64_t n, int32_t size, int32_t *dist_dev,
                          int16_t *field_dev, void *stream);
/* The same kernel on the context's current state: dist_dev int32[N], field_dev (nullable) int16[N][4][size][size].
 * Reads the maps and poses only: no look-ahead slot, RNG or env state changes. */
int merlin_env_optimal_steps(merlin_env *env, int32_t *dist_dev, int16_t *field_dev, void *stream);
/* [host] merlin_shortest_paths on host arrays (query q uses map q), a queue search in plain C++: the library's
 * CPU-side restatement of the kernel.  field nullable. */
int merlin_shortest_paths_host(const uint32_t *walls, const int32_t *goal, const int32_t *agent, int64_t n,
                               int32_t size, int32_t *dist, int16_t *field);
/* The policy field (no reference counterpart).  A policy that acts on the view codes alone, by the
 * argmax, turns a map into a functional graph over its 4 size^2 poses: the two entries below are what that needs
 * beside the policy's own forward.
 * Stateless observation codes, in merlin_render_frames' layouts: query q < n shows map m = map_index_dev[q] (NULL: q)
 * -- walls_dev uint32[M][size], goal_dev int32[M][2] (NULL or a position outside the grid: no goal) -- from the pose
 * agent_dev[q] int32[4] = (x, y, dir, 0).  codes_dev uint32[n][MERLIN_OBS_WORDS]: bit for bit the words
 * merlin_env_reset / merlin_env_step write for an env in that state (any 4-B alignment; 16 B takes wider stores).
 * A pose outside the grid, on a wall or with dir outside 0..3 has no view: its 8 words are zero (no agent tile:
 * merlin_tower_codes_conv3 flags such a row as MERLIN_DEVERR_BAD_TILE) and MERLIN_DEVERR_BAD_FRAME is raised
 * (merlin_tower_errors).  size outside 5..32, negative n or a null required pointer: MERLIN_E_INVALID; n = 0 is a
 * no-op.  map_index_dev's values are the caller's to keep inside [0, M).  One kernel, no allocation, no host sync:
 * capturable (after the device's first library call, which allocates the error word). */
int merlin_view_codes(const uint32_t *walls_dev, const int32_t *goal_dev, const int32_t *agent_dev,
                      const int32_t *map_index_dev, int64_t n, int32_t size, uint32_t *codes_dev, void *stream);
/* action_dev int8[n_maps][4][size][size], indexed [dir][y][x] as the distance field: the action each pose takes.
 * steps_dev int16[n_maps][4][size][size]: steps(p) = the number of actions after which an episode started in pose p
 * terminates when every pose takes its own action under the step rule above (merlin_shortest_paths), -1 if it never
 * does: a cycle, a forward move into a wall or off the grid, a pose on a wall, an action outside {0, 1, 2}, and
 * every pose that leads to one of those.  No horizon is applied (values are at most 4 size^2 <= 4,096; compare with
 * max_steps).  The goal cell is an ordinary free cell for a pose standing on it, and a free pose in front of the
 * goal whose action is forward has steps 1 whatever the pose on the goal cell does.  A goal outside the grid: -1
 * everywhere.  With a shortest-path action at every pose, steps equals merlin_shortest_paths' field.  Any 2-B
 * alignment of steps_dev.  size outside 5..32, negative n_maps or a null pointer: MERLIN_E_INVALID; n_maps = 0 is a
 * no-op.  One kernel, no allocation, no host sync: capturable. */
int merlin_policy_paths(const uint32_t *walls_dev, const int32_t *goal_dev, const int8_t *action_dev,
                        int64_t n_maps, int32_t size, int16_t *steps_dev, void *stream);
/* [host] merlin_policy_paths on host arrays by another algorithm, a forward walk per pose with memoisation and cycle
 * marks in plain C++: the library's CPU-side restatement of the kernel. */
int merlin_policy_paths_host(const uint32_t *walls, const int32_t *goal, const int8_t *action, int64_t n_maps,
                             int32_t size, int16_t *steps);
/* The sampled-policy field (no reference counterpart).  A policy that SAMPLES its action from
 * probabilities which depend on the view codes alone turns a map into a time-homogeneous Markov chain over its
 * 4 size^2 poses; the two entries below are its dynamic programmes over the horizon, exact where a rollout is noisy.
 * Dynamics: merlin_env_step's rule, unshaped (no StuckPenalty, no ExplorationBonus).  Action 0 turns left
 * ((d + 3) & 3), 1 turns right ((d + 1) & 3), 2 moves forward: a front cell that is the goal terminates the episode,
 * one that is a wall or off the grid leaves the pose unchanged (a self loop, not a dead end).  Action number t earns
 * r_t = 1.0 - 0.9 * ((double)t / (double)T) if it terminates, and the episode is truncated after T = horizon actions.
 * The goal cell is an ordinary free cell for a pose standing on it; a goal outside the grid: nothing terminates.
 * probs_dev float32[n_maps][4][size][size][3], indexed [map][dir][y][x][action]; values at wall poses are ignored.
 * The kernels widen to double and normalise, q_a = p_a / ((p_0 + p_1) + p_2) (float32 softmax rows do not sum to 1).
 * A free pose whose row has a negative or non-finite entry or sums to zero is the caller's to keep out: not checked.
 *
 * Backwards: h_t(p) = the probability that an episode started in pose p at step count 0 terminates at exactly action t,
 *   h_1(p) = q_F(p) [front(p) is the goal],  h_{t+1}(p) = (q_L(p) h_t(left p) + q_R(p) h_t(right p)) + q_F(p) g_t(p),
 *   g_t(p) = 0 if front(p) is the goal, h_t(p) if it is a wall or off the grid, h_t(fwd p) otherwise.
 * Outputs float64[n_maps][4][size][size], each nullable (not all), 8-B aligned, accumulated over t = 1..T:
 *   success = sum h_t;  ret = sum h_t r_t;  steps = sum t h_t + T (1 - success), the expected episode length;
 *   disc = sum h_t (G_t r_t), G_1 = 1, G_{t+1} = G_t gamma (a running product), the discounted return from step 0.
 * Wall poses get NaN in all four.  size outside 5..32, horizon outside 1..16384, negative n_maps, a null input or all
 * outputs null: MERLIN_E_INVALID; n_maps = 0 is a no-op.  One kernel, no allocation, no host sync: capturable. */
int merlin_policy_chain(const uint32_t *walls_dev, const int32_t *goal_dev, const float *probs_dev, int64_t n_maps,
                        int32_t size, int32_t horizon, double gamma, double *success_dev, double *ret_dev,
                        double *steps_dev, double *disc_dev, void *stream);
/* Forwards from one start pose per map, agent_dev int32[n_maps][4] = (x, y, dir, 0): mu_0 = the start pose, mu_{t+1}
 * the chain's push-forward of mu_t, computed as a gather -- pose (x, y, d) receives mass from (x, y, (d + 1) & 3) by a
 * left turn, from (x, y, (d + 3) & 3) by a right turn, from the free cell behind it by a forward move unless (x, y)
 * is the goal, and from itself by a forward move if its front is blocked.
 *   visits_dev float64[n_maps][4][size][size] = sum over t = 0..T-1 of mu_t, 0.0 at wall poses;
 *   hit_dev float64[n_maps][T]: hit[m][t - 1] = the probability that the episode terminates at action t, summed over
 *   the at most four poses facing the goal in the order d = 0..3.
 * Each nullable (not both), 8-B aligned.  With the backward pass: sum_t hit = success[start], sum_t hit r_t =
 * ret[start], sum_p visits = steps[start].  A start pose off the grid, on a wall or with dir outside 0..3 fills that
 * map's outputs with NaN and raises MERLIN_DEVERR_BAD_FRAME (merlin_tower_errors), as merlin_view_codes does.
 * Argument rules as merlin_policy_chain.  One kernel, no allocation, no host sync: capturable (after the device's
 * first library call, which allocates the error word). */
int merlin_policy_occupancy(const uint32_t *walls_dev, const int32_t *goal_dev, const float *probs_dev,
                            const int32_t *agent_dev, int64_t n_maps, int32_t size, int32_t horizon,
                            double *visits_dev, double *hit_dev, void *stream);
/* [host] the two passes on host arrays by another route, a recursion / a scatter over an explicit successor table
 * with three entries per pose and one absorbing state, in plain C++: the library's CPU-side restatements of the
 * kernels.  An invalid start pose fills its map's outputs with NaN (there is no error word on the host). */
int merlin_policy_chain_host(const uint32_t *walls, const int32_t *goal, const float *probs, int64_t n_maps,
                             int32_t size, int32_t horizon, double gamma, double *success, double *ret,
                             double *steps, double *disc);
int merlin_policy_occupancy_host(const uint32_t *walls, const int32_t *goal, const float *probs,
                                 const int32_t *agent, int64_t n_maps, int32_t size, int32_t horizon,
                                 double *visits, double *hit);
/* [sync] read-and-clear the device error bits and the fallback-map counter. */
int merlin_env_errors(merlin_env *env, uint32_t *flags_host, uint32_t *fallbacks_host,
                      void *stream);
int merlin_env_num_envs(const merlin_env *env);
int merlin_env_size(const merlin_env *env);

/* Observation expansion: out[k] = RGB image of codes_dev[index_dev ? index_dev[k] : k],
 * k < n.  f32: values are tile bytes * scale (scale = 1/255 folds
 * CNNFeatureExtractor's /255), layout MERLIN_LAYOUT_*.  u8: NHWC bytes, exactly
 * the RGBImgPartialObsWrapper(tile_size=8) frame. */
int merlin_obs_expand_f32(const uint32_t *codes_dev, const int64_t *index_dev, int64_t n,
                          float *out_dev, float scale, int32_t layout, void *stream);
int merlin_obs_expand_u8(const uint32_t *codes_dev, const int64_t *index_dev, int64_t n,
                         uint8_t *out_dev, void *stream);

/* GAE over [T][N] (row t, env i at t*N+i), truncation treated as terminal
 * (done = term or trunc).  stats_dev (nullable) receives double[3] =
 * (count, sum adv, sum adv^2) of this call's advantages -- the per-rank
 * partial that multi-GPU callers all-reduce before merlin_adv_normalize. */
int merlin_gae(const float *reward_dev, const float *value_dev, const float *done_dev,
               const float *last_value_dev, float *adv_dev, float *ret_dev, int32_t T, int32_t N,
               double gamma, double lam, double *stats_dev, void *stream);
/* out[k] = (adv[k] - mean) / (std_unbiased + 1e-8) with mean/std from
 * stats_dev = (count, sum, sum of squares); out may alias adv. */
int merlin_adv_normalize(const float *adv_dev, int64_t n, const double *stats_dev, float *out_dev,
                         void *stream);

/* conv1 from tile codes (both towers at once).  tables_dev: float[towers][32][4][20]
 * = P[co][slot=(dy,dx)][class*4 + quarter], the conv1 weights contracted with the
 * /255-scaled atlas (see csrc/merlin_conv1.hip); bias_dev float[towers][32].
 * out_dev float[towers][n][32][13][13] = relu(conv1(frame_k)) with frame_k the frame
 * of codes_dev[index_dev ? index_dev[k] : k]. */
int merlin_conv1_lut_fwd(const uint32_t *codes_dev, const int64_t *index_dev, int64_t n,
                         const float *tables_dev, const float *bias_dev, int32_t towers,
                         float *out_dev, void *stream);
/* Backward: dz = grad * (act > 0) with act/grad float[towers][n][32][13][13];
 * writes dtables_dev float[towers][32][4][20] and dbias_dev float[towers][32]
 * (overwritten, not accumulated). */
int merlin_conv1_lut_bwd(const uint32_t *codes_dev, const int64_t *index_dev, int64_t n,
                         const float *act_dev, const float *grad_dev, int32_t towers,
                         float *dtables_dev, float *dbias_dev, void *stream);

/* Tower stages (towers = 1 or 2; n frames; K orders are (ky, kx, ci)).
 * conv2_im2col_fwd: A2[t][k*25 + p2][(ky*4+kx)*32 + ci] = relu(conv1 of frame k)[ci]
 *   at (2*oy+ky, 2*ox+kx), p2 = oy*5+ox; tables/bias as merlin_conv1_lut_fwd.
 * conv2_im2col_bwd: dtables/dbias of that map given dA2 (same layout); the ReLU mask
 *   is recomputed from the tables.
 * conv3_im2col_fwd: A3[t][k*9 + p3][(ky*3+kx)*64 + ci] = relu(Z2[t][k*25 + (oy+ky)*5
 *   + ox+kx][ci] + b2[t][ci]), p3 = oy*3+ox.
 * conv3_col2im_bwd: dZ2 = [Z2 + b2 > 0] * col2im(dA3). */
int merlin_tower_conv2_im2col_fwd(const uint32_t *codes_dev, const int64_t *index_dev, int64_t n,
                                  const float *tables_dev, const float *bias_dev, int32_t towers,
                                  float *A2_dev, void *stream);
int merlin_tower_conv2_im2col_bwd(const uint32_t *codes_dev, const int64_t *index_dev, int64_t n,
                                  const float *tables_dev, const float *bias_dev,
                                  const float *dA2_dev, int32_t towers, float *dtables_dev,
                                  float *dbias_dev, void *stream);
int merlin_tower_conv3_im2col_fwd(const float *Z2_dev, const float *b2_dev, int64_t n,
                                  int32_t towers, float *A3_dev, void *stream);
int merlin_tower_conv3_col2im_bwd(const float *dA3_dev, const float *Z2_dev, const float *b2_dev,
                                  int64_t n, int32_t towers, float *dZ2_dev, void *stream);
/* Same, writing dZ2 chunk-major, dZ2c[t][ci/4][k*25 + p2][ci%4] (the histogram's input),
 * and absmax_dev[0] = float bits of max |dZ2| (the histogram's fixed-point scale). */
int merlin_tower_conv3_col2im_bwd_chunked(const float *dA3_dev, const float *Z2_dev,
                                          const float *b2_dev, int64_t n, int32_t towers,
                                          float *dZ2c_dev, uint32_t *absmax_dev, void *stream);

/* conv1 + conv2 as table lookups (csrc/merlin_conv2lut.hip has the derivation).
 * tables_dev float[towers][rows][64], rows = merlin_tower_conv2_lut_rows() = 2720:
 *   row = base(type) + 4*v + j for conv2 tap (ky, kx), type = (ky&1, kx&1) with bases
 *   0 / 20 / 120 / 220 for (0,0) / (0,1) / (1,0) / (1,1), j = 2*(ky>>1) + (kx>>1), and v
 *   the classes of the tiles the tap's conv1 position covers, in base 5 (row-major tiles).
 *   Row content: W2[:, :, ky, kx] applied to relu(conv1) of that tile combination.
 * lut_fwd: Z2[t][k*25 + p2][co] = sum over the 16 taps of tables[t][row(tap, p2, frame k)][co]
 *   (conv2 of relu(conv1(frame k)), no conv2 bias), frame k = codes[index ? index[k] : k].
 * lut_bwd: dtables[t][row][co] = sum of dZ2 over the (k, p2) that read row at some tap, for
 *   frame k = codes_dev[k] (the minibatch's own rows, no index), given dZ2 chunk-major and its
 *   max |dZ2| (float bits, >= the true max) as written by
 *   merlin_tower_conv3_col2im_bwd_chunked; summed in 64-bit fixed point (exact,
 *   order-independent), overwritten, not accumulated.  A non-finite max gives NaN. */
int merlin_tower_conv2_lut_rows(void);
int merlin_tower_conv2_lut_fwd(const uint32_t *codes_dev, const int64_t *index_dev, int64_t n,
                               const float *tables_dev, int32_t towers, float *Z2_dev,
                               void *stream);
int merlin_tower_conv2_lut_bwd(const uint32_t *codes_dev, int64_t n, const float *dZ2c_dev,
                               const uint32_t *absmax_dev, int32_t towers, float *dtables_dev,
                               void *stream);
/* Grouped form (one weight set per group of frames: FOMAML's per-task policies, src/fomaml.py:158-212).
 * towers = 2 * groups; frames codes[g * group_frames + i] (i < group_frames) belong to group g and are
 * evaluated by towers 2g (actor) and 2g+1 (critic) only, with their own tables:
 * lut_fwd_grouped: Z2[2g + c][i*25 + p2][co] for the n = groups * group_frames frames;
 * lut_bwd_grouped: dtables[2g + c] from dZ2c[2g + c] (chunk-major, group_frames frames per tower, as
 *   merlin_tower_conv3_col2im_bwd_chunked writes it for n = group_frames, towers = 2 * groups);
 *   slabs_dev: caller-owned scratch of merlin_tower_conv2_lut_slab_bytes(towers, group_frames) bytes. */
int merlin_tower_conv2_lut_fwd_grouped(const uint32_t *codes_dev, int64_t n, int64_t group_frames,
                                       const float *tables_dev, int32_t towers, float *Z2_dev, void *stream);
int64_t merlin_tower_conv2_lut_slab_bytes(int32_t towers, int64_t group_frames);
int merlin_tower_conv2_lut_bwd_grouped(const uint32_t *codes_dev, int64_t group_frames, const float *dZ2c_dev,
                                       const uint32_t *absmax_dev, int32_t towers, float *dtables_dev,
                                       void *slabs_dev, void *stream);

/* Receptive-field windows (csrc/merlin_window.hip; the plan is built by merlin/windows.py).
 * window_lut:   Z2w[t][w][co] = sum over the 16 taps of tables[t][rows[w][tap]][co]
 *               (rows int32[n_windows][16]: conv2 table rows as merlin_tower_conv2_lut_fwd's)
 * window_conv3: Y3[t][k*9 + p3][co] = relu(b3[t][co] + sum over tap = ky*3 + kx of
 *               Q[t][wid[g*25 + (oy+ky)*5 + ox+kx]][tap][co]), g = groups ? groups[k] : k,
 *               p3 = oy*3 + ox; Q float[towers][n_windows][9][64], wid int32[*][25]
 * segment_sum:  out[t][key[e]][:] = sum over the nnz entries e (keys ascending) of
 *               src[t][row(e)][:], each destination summed in entry order (no atomics);
 *               row(e) = idx[e], or with slot_dev slot[idx[e] / sub] * sub + idx[e] % sub,
 *               entries whose slot is -1 skipped.  Items of item_len entries; fix_dev
 *               int32[n_fix][4] = (dst, first item, last item, carry slot in the first item)
 *               for destinations spanning items; carry_dev float[towers][ceil(nnz /
 *               item_len)][2][64] scratch.  out float[towers][out_rows][64] is overwritten
 *               (rows without entries = 0), or with accumulate != 0 the sums are added to it
 *               (a list split by source block into several calls sums in call order). */
int merlin_tower_window_lut(const int32_t *rows_dev, int64_t n_windows, const float *tables_dev,
                            int32_t towers, float *Z2w_dev, void *stream);
/* The live-patch maps of every minibatch of an update (merlin/windows.py WindowPlan._bulk_minibatches): group g
 * (group_keys[g] = minibatch m * n_frames + frame; group_offsets[m] = first group of minibatch m), position p3 ->
 * patch k = kid[frame * 9 + p3]: kmap[m * n_patches + k] = k (preset to -1 by the caller), rmap[...] = one row
 * j * 9 + p3 of m holding k (scratch, no preset), rep_row[g * 9 + p3] = that row (conv3's patch representatives). */
int merlin_minibatch_patch_maps(const int32_t *kid_dev, const int64_t *group_keys_dev, int64_t n_groups,
                                int64_t n_frames, const int64_t *group_offsets_dev, int32_t n_patches, int32_t *kmap_dev,
                                int32_t *rmap_dev, int32_t *rep_row_dev, void *stream);
/* Every minibatch's grouping arrays of an update in one stable sort, one scan and one pass (merlin/windows.py
 * WindowPlan.update_minibatches(bulk=True) builds the same arrays with torch, element for element).  idxs_dev int64[n]:
 * the epochs' permutations back to back, n a multiple of period; each period is cut into minibatches of `minibatch`
 * samples (the last may be short), numbered m = 0 .. nmb - 1 across the epochs.  uid_dev int64[n_samples]: frame id
 * in [0, n_frames) of each sample.  With G = the number of distinct (minibatch, frame) pairs, in (m, frame) order:
 *   group_keys[G] = m * n_frames + frame, groups[G] = frame          (both sized n by the caller)
 *   group_offsets int64[nmb + 2]: [m] = first group of m, [nmb] = G, [nmb + 1] = 1 if an index of idxs or a frame id
 *                 of uid was out of range (it was then taken as frame 0), else 0
 *   inv int64[n]: [pos] = position of sample pos's frame among its minibatch's groups
 *   slot int32[nmb][n_frames]: that position per frame, -1 for a frame absent from the minibatch
 *   order int32[n]: per minibatch (its samples are sorted positions lo .. hi of the update), the sample positions
 *                 within the minibatch grouped by frame, ascending within a frame
 *   offs int32[G + nmb] (sized n + nmb): minibatch m's CSR row starts at offs[group_offsets[m] + m], count + 1 entries
 * workspace_dev: merlin_plan_minibatches_workspace bytes (-1: bad arguments) of device memory, contents free between
 * calls; no allocation happens inside.  n and nmb * n_frames must be below 2^31 (MERLIN_E_UNSUPPORTED). */
int64_t merlin_plan_minibatches_workspace(int64_t n, int64_t period, int64_t minibatch, int64_t n_frames);
/* The update's frame groups, window / patch / band numbering and the four segmented-sum lists (merlin/dedup.py
 * FrameGroups, merlin/windows.py WindowPlan and SegmentPlan build the same arrays with torch, element for element; only
 * rep, any member of its group, is free).  Five stages, each one stable radix sort of (key, entry index) pairs, the run
 * ids being the numbering and the sorted order the list; a stage's list length comes from the stage before, so the
 * caller reads counts_dev (int64[8]: frames, mismatch flag, windows, table-row flag, patches, bands, missing-window
 * flag) after frames, after patches and after bands.  Every stage sorts in workspace_dev, at least
 * merlin_plan_sort_workspace(list length, key bytes) bytes (frames: n, 8; windows: 16 n_windows, 4; patches:
 * 9 n_frames, 8; bands: 3 n_patches, 8; dq: 3 n_bands, 4); nothing is allocated inside.
 *   frames   codes uint32[n][8], mult_host: the 8 hash multipliers (host memory) -> uid int64[n] (groups numbered by
 *            ascending signed hash), rep int64[n] (first n_frames written), wkey int32[n][25] / pkey uint64[n][9] (the
 *            representatives' window and patch keys, first n_frames rows), mark / wrank int32[5^9] (the window keys
 *            present and their ranks), counts[0..2]; counts[1] = 1 when a frame differs from its representative
 *   windows  -> wid int32[n_frames][25], rows int32[n_windows][16] (counts[3] = 1 when a row >= lut_rows) and the dT2
 *            list (16 n_windows entries: key = table row, idx = window)
 *   patches  -> kid int32[n_frames][9], pk uint64[9 n_frames] (the distinct patch keys, counts[4] of them) and the
 *            patch list (9 n_frames entries)
 *   bands    -> ub uint64[3 n_patches] (the distinct (row, band) keys, counts[5]) and the band list (3 n_patches)
 *   dq       -> the dQ list (3 n_bands entries: key = Q row w * 9 + tap, idx = band)
 * Each list: key / idx int32[entries], fix int32[items][4] and head_fix int32[items] for items of item_len entries
 * (merlin_segment_sum's fix rows). */
int64_t merlin_plan_sort_workspace(int64_t n, int32_t key_bytes);
int merlin_plan_frames(const uint32_t *codes_dev, int64_t n, const uint64_t *mult_host, void *workspace_dev,
                       int64_t workspace_bytes, int64_t *uid_dev, int64_t *rep_dev, int32_t *wkey_dev,
                       uint64_t *pkey_dev, int32_t *mark_dev, int32_t *wrank_dev, int64_t *counts_dev, void *stream);
int merlin_plan_windows(int64_t n_frames, int64_t n_windows, const int32_t *wkey_dev, const int32_t *mark_dev,
                        const int32_t *wrank_dev, int32_t lut_rows, int64_t item_len, void *workspace_dev,
                        int64_t workspace_bytes, int32_t *wid_dev, int32_t *rows_dev, int32_t *key_dev,
                        int32_t *idx_dev, int32_t *fix_dev, int32_t *head_fix_dev, int64_t *counts_dev, void *stream);
int merlin_plan_patches(int64_t n_frames, const uint64_t *pkey_dev, int64_t item_len, void *workspace_dev,
                        int64_t workspace_bytes, int32_t *kid_dev, uint64_t *pk_dev, int32_t *key_dev,
                        int32_t *idx_dev, int32_t *fix_dev, int32_t *head_fix_dev, int64_t *counts_dev, void *stream);
int merlin_plan_bands(int64_t n_patches, const uint64_t *pk_dev, int64_t item_len, void *workspace_dev,
                      int64_t workspace_bytes, uint64_t *ub_dev, int32_t *key_dev, int32_t *idx_dev, int32_t *fix_dev,
                      int32_t *head_fix_dev, int64_t *counts_dev, void *stream);
int merlin_plan_dq(int64_t n_bands, int64_t n_windows, const uint64_t *ub_dev, const int32_t *mark_dev,
                   const int32_t *wrank_dev, int64_t item_len, void *workspace_dev, int64_t workspace_bytes,
                   int32_t *key_dev, int32_t *idx_dev, int32_t *fix_dev, int32_t *head_fix_dev, int64_t *counts_dev,
                   void *stream);
int merlin_plan_minibatches(const int64_t *idxs_dev, int64_t n, int64_t period, int64_t minibatch,
                            const int64_t *uid_dev, int64_t n_samples, int64_t n_frames, void *workspace_dev,
                            int64_t workspace_bytes, int64_t *group_keys_dev, int64_t *groups_dev, int64_t *inv_dev,
                            int32_t *slot_dev, int32_t *order_dev, int32_t *offs_dev, int64_t *group_offsets_dev,
                            void *stream);
/* window_lut with conv2's bias and ReLU applied as the rows are written: a2w[t][w] = relu(Z2w[t][w] + b2[t]). */
int merlin_tower_window_lut_bias_relu(const int32_t *rows_dev, int64_t n_windows, const float *tables_dev,
                                      int32_t towers, const float *b2_dev, float *a2w_dev, void *stream);
int merlin_tower_window_conv3(const float *Q_dev, int64_t n_windows, const int32_t *wid_dev,
                              const int64_t *groups_dev, int64_t n, const float *b3_dev,
                              int32_t towers, float *Y3_dev, void *stream);
/* conv3 of the acting path from a table over every 3x3 tile window an observation can hold:
 * Qall_dev float[towers][merlin_tower_all_windows() = 4^9 + 3 * 4^8 = 458,752][9][64] (Q of
 * merlin_tower_window_conv3 for the window with compact key k: a window away from the agent's view cell (3, 6) =
 * its 9 tile classes 0..3 in base 4, tile (0,0) most significant; a window at conv2 position (4, wx), wx = 1..3,
 * which holds the agent's tile (class 4) at local (2, 3 - wx) = 4^9 + (wx - 1) 4^8 + its other 8 classes in
 * base 4 -- merlin/windows.py compact_window_keys; built once per rollout, merlin/actor_critic.py rollout_pack);
 * Y3[t][k*9 + p3][co] = relu(b3[t][co] + sum over the 9 taps of Qall[t][id of frame k's window at
 * p3 + tap][tap][co]) for frames codes_dev[k] (8 words of tile-class nibbles, merlin_env_step). */
int64_t merlin_tower_all_windows(void);
int merlin_tower_codes_conv3(const uint32_t *codes_dev, int64_t n, const float *Qall_dev,
                             const float *b3_dev, int32_t towers, float *Y3_dev, void *stream);
/* Same, with amax_dev (or NULL): atomicMax of max |Y3| per tower as float bits into amax_dev[t] (zeroed by the
 * caller), the operand scale of the acting path's fc1 on merlin_h3_gemm_nt. */
int merlin_tower_codes_conv3_amax(const uint32_t *codes_dev, int64_t n, const float *Qall_dev,
                                  const float *b3_dev, int32_t towers, float *Y3_dev, uint32_t *amax_dev,
                                  void *stream);
/* tower_errors: the device error flags the tower kernels raised on this device since the last call
 * (MERLIN_DEVERR_BAD_TILE from merlin_tower_codes_conv3: a frame whose compact table key is not its window), then
 * clears them; synchronises `stream` (PPO reads it once per rollout, with merlin_env_errors). */
int merlin_tower_errors(uint32_t *flags, void *stream);
/* Same, also writing relu_bits_dev uint64[towers][n*9]: bit co of row (k*9 + p3) = Y3 > 0 there; amax_dev
 * (or NULL): atomicMax of max |Y3| per tower as float bits into amax_dev[t] (zeroed by the caller), the operand
 * scale of fc1's f16 two-plane GEMMs (merlin_h3_gemm_*). */
int merlin_tower_window_conv3_bits(const float *Q_dev, int64_t n_windows, const int32_t *wid_dev,
                                   const int64_t *groups_dev, int64_t n, const float *b3_dev,
                                   int32_t towers, float *Y3_dev, uint64_t *relu_bits_dev, uint32_t *amax_dev,
                                   void *stream);
/* merlin_tower_window_conv3_bits (relu_bits_dev may be NULL here) computing each distinct 5x5-tile patch once:
 * rows (k, p3) whose frames hold the same patch at p3 read the same windows, so only the representative rows
 * (rep_row_dev[r] == r; rep_row_dev int32[n*9]: for every row r = k*9 + p3 of this call, a row of this call holding
 * the same patch, itself a representative) are computed; a second launch copies the other rows from theirs: their
 * Y3 rows with copy bit 0, their mask words with copy bit 1 (copy = 3: the same outputs as _bits; without a bit
 * the non-representative rows stay unwritten, for consumers that read rows through rep_row_dev); copy bit 2: the
 * copies only, after a call that computed the representatives (e.g. on another stream). */
int merlin_tower_window_conv3_reuse(const float *Q_dev, int64_t n_windows, const int32_t *wid_dev,
                                    const int64_t *groups_dev, int64_t n, const float *b3_dev,
                                    int32_t towers, float *Y3_dev, uint64_t *relu_bits_dev, uint32_t *amax_dev,
                                    const int32_t *rep_row_dev, int32_t copy, void *stream);
/* window_conv3_planes: window_conv3_reuse with copy = 0 (representatives only; the bits of the other rows are read
 * through rep_row by merlin_segment_sum_mask_rows) writing Y3 as its h3 planes (Y3_planes [t][n*9][8][2][8] f16, the
 * fp32 Y3's byte layout) for fc1's plane-operand GEMMs.  The plane scale of tower t comes from a bound on max Y3
 * computed first from Q: bound[t] (written, float bits) = max over c of relu(b3[t][c] + sum over taps of
 * max_w Q[t][w][tap][c]) >= every Y3 value; colmax_ws uint32[towers * 64 * 576] is scratch (per-block column maxima). */
int merlin_tower_window_conv3_planes(const float *Q_dev, int64_t nw, const int32_t *wid_dev, const int64_t *groups_dev,
                                     int64_t n, const float *b3_dev, int32_t towers, void *Y3_planes_dev,
                                     uint64_t *relu_bits_dev, const int32_t *rep_row_dev, uint32_t *colmax_ws_dev,
                                     uint32_t *bound_dev, void *stream);
int merlin_segment_sum(const float *src_dev, int64_t src_rows, const int32_t *idx_dev,
                       const int32_t *key_dev, int64_t nnz, const int32_t *slot_dev, int32_t sub,
                       int64_t item_len, const int32_t *fix_dev, int64_t n_fix, int32_t towers,
                       float *out_dev, int64_t out_rows, float *carry_dev, int32_t accumulate,
                       void *stream);
/* merlin_segment_sum with options.  mask_dev (or NULL): each source row is multiplied by a ReLU
 * mask of the same row (src where mask > 0, else 0: the ReLU backward of a forward output,
 * fused into the gather); float[towers][src_rows][64], or with MERLIN_SEG_MASK_BITS
 * uint64[towers][src_rows] (bit ch = channel ch > 0, as merlin_tower_window_conv3_bits writes).
 * flags: MERLIN_SEG_ACCUMULATE as accumulate != 0 above; MERLIN_SEG_NO_FILL leaves the rows of
 * destinations without any (unskipped) entry untouched instead of zeroing them (the caller
 * knows which rows are live, e.g. merlin/windows.py's patch sums). */
#define MERLIN_SEG_ACCUMULATE 1
#define MERLIN_SEG_NO_FILL 2
#define MERLIN_SEG_MASK_BITS 4
/* bits 8..10: which pass of conv3's backward this is (1 R, 2 S, 3 dQ, 4 dT2; 0 generic) -- it only
 * names the kernel instantiation, so profiles tell the passes apart; the sums are the same */
#define MERLIN_SEG_ROLE_SHIFT 8
#define MERLIN_SEG_ROLE_MASK (7 << MERLIN_SEG_ROLE_SHIFT)
int merlin_segment_sum_masked(const float *src_dev, const void *mask_dev, int64_t src_rows,
                              const int32_t *idx_dev, const int32_t *key_dev, int64_t nnz,
                              const int32_t *slot_dev, int32_t sub, int64_t item_len,
                              const int32_t *fix_dev, int64_t n_fix, int32_t towers, float *out_dev,
                              int64_t out_rows, float *carry_dev, int32_t flags, void *stream);
/* merlin_segment_sum_masked that also marks the destinations it sums into: mark_dev int32[out_rows]
 * (or NULL), mark[key(e)] = key(e) for every entry e not skipped; rows of other keys keep what the
 * caller put there (-1).  The marks are a slot map (sub 1) for a following pass that reads these
 * rows, so it skips the rows no entry was summed into (with MERLIN_SEG_NO_FILL they are never
 * written: merlin/fast_step.py's band sums of conv3's backward). */
int merlin_segment_sum_marked(const float *src_dev, const void *mask_dev, int64_t src_rows,
                              const int32_t *idx_dev, const int32_t *key_dev, int64_t nnz,
                              const int32_t *slot_dev, int32_t sub, int64_t item_len,
                              const int32_t *fix_dev, int64_t n_fix, int32_t towers, float *out_dev,
                              int64_t out_rows, float *carry_dev, int32_t flags, int32_t *mark_dev,
                              void *stream);
/* merlin_segment_sum_marked with the destinations that span items finished inside the launch (no second fix-up
 * launch): head_fix_dev int32[n_items] = the fix row (the item) at which item i's first destination started when it
 * continues into item i, else -1; counters_dev int32[n_fix] zero before the first call (the launch leaves them zero).
 * Requires one fix row per item (n_fix = ceil(nnz / item_len), as merlin/windows.py SegmentPlan builds it).  The
 * item that completes a row adds the row's partial sums in the fix-up pass's order: the same bits as
 * merlin_segment_sum_marked.  Both NULL: that function. */
int merlin_segment_sum_fused(const float *src_dev, const void *mask_dev, int64_t src_rows,
                             const int32_t *idx_dev, const int32_t *key_dev, int64_t nnz,
                             const int32_t *slot_dev, int32_t sub, int64_t item_len,
                             const int32_t *fix_dev, int64_t n_fix, int32_t towers, float *out_dev,
                             int64_t out_rows, float *carry_dev, int32_t flags, int32_t *mark_dev,
                             const int32_t *head_fix_dev, int32_t *counters_dev, void *stream);
/* merlin_segment_sum_fused with the mask's bit words read through a row map: the mask of source row r is
 * mask[t][mask_rows[r]] (conv3's patch representatives, merlin_tower_window_conv3_reuse with copy = 0: rows of one
 * patch share their ReLU mask and only the representatives' words are written). */
int merlin_segment_sum_mask_rows(const float *src_dev, const void *mask_dev, int64_t src_rows, const int32_t *idx_dev,
                                 const int32_t *key_dev, int64_t nnz, const int32_t *slot_dev, int32_t sub,
                                 int64_t item_len, const int32_t *fix_dev, int64_t n_fix, int32_t towers, float *out_dev,
                                 int64_t out_rows, float *carry_dev, int32_t flags, int32_t *mark_dev,
                                 const int32_t *head_fix_dev, int32_t *counters_dev, const int32_t *mask_rows_dev,
                                 void *stream);

/* Acting tail (src/actor_critic.py:48-55 act, src/ppo.py:69-71): z float[2][n][hidden] = fc1's
 * pre-activation of the actor / critic tower, b4 float[2][hidden]; h = relu(z + b4); logits =
 * w_actor float[act_dim][hidden] . h0 + b_actor, value = w_critic float[hidden] . h1 + b_critic[0];
 * action int64[n] = argmax(logits) when deterministic, else a Categorical(logits) draw (exponential
 * races on a counter-based generator keyed by seed, *epoch_dev (NULL = 0; bump it to redraw in
 * a replayed graph), step and the global env index env_offset + k, so data-parallel shards draw
 * what one process over the concatenated envs draws); logp float[n] = log_softmax(logits)[action],
 * value float[n].  hidden % 4 == 0, act_dim <= 8.  Non-finite logits (where the reference's
 * Categorical(logits) raises) give action -1, which merlin_env_step flags as
 * MERLIN_DEVERR_BAD_ACTION. */
int merlin_act_heads(const float *z_dev, const float *b4_dev, int64_t n, int32_t hidden,
                     const float *w_actor_dev, const float *b_actor_dev, const float *w_critic_dev,
                     const float *b_critic_dev, int32_t act_dim, int32_t deterministic, uint64_t seed,
                     const int64_t *epoch_dev, int64_t step, int64_t env_offset, int64_t *action_dev,
                     float *logp_dev,
                     float *value_dev, void *stream);

/* PPO minibatch loss (src/ppo.py:136-150), per distinct frame u < n_frames of the minibatch:
 *   logits float[n_frames][act_dim] (act_dim <= 8), value float[n_frames]; the frame's samples
 *   are order[offs[u] .. offs[u+1]) (int32 CSR, offs[n_frames] = n_samples, every frame owns
 *   >= 1 sample), frame_of int64[n_samples] maps a sample to its frame (frame_of[order[k]] =
 *   the u whose range holds k), and sample i reads actions / logp_old / adv / ret at
 *   sample_index[i] (int64; NULL = i).  With logp = log_softmax(logits), ratio = exp(logp[a] -
 *   logp_old),
 *   loss = -mean(min(ratio*A, clamp(ratio, 1-clip_eps, 1+clip_eps)*A)) + vf_coef*mean((v-R)^2)
 *          - ent_coef*mean(entropy)
 * writes loss float[1], dlogits float[n_frames][act_dim] and dvalue float[n_frames] = d loss /
 * d (logits, value) summed over each frame's samples (fixed order; torch.min / clamp
 * subgradients), and adds (-mean(min(...)), mean((v-R)^2), mean(entropy), mean(logp_old -
 * logp), mean(|ratio-1| > clip_eps)) to stats double[5] (NULL: not written).  workspace double[
 * merlin_ppo_loss_workspace(n_samples)].  An action outside [0, act_dim) makes the loss NaN.
 * bias_actor float[act_dim] / bias_critic float[1] (NULL = 0) are added to logits / value
 * first, and dbias_actor / dbias_critic (NULL: not written) get their gradients. */
int64_t merlin_ppo_loss_workspace(int64_t n_samples);
int merlin_ppo_loss(const float *logits_dev, const float *value_dev, const float *bias_actor_dev,
                    const float *bias_critic_dev, int64_t n_frames, int32_t act_dim, const int32_t *offs_dev,
                    const int32_t *order_dev, const int64_t *frame_of_dev, int64_t n_samples,
                    const int64_t *sample_index_dev, const int64_t *actions_dev, const float *logp_old_dev,
                    const float *adv_dev, const float *ret_dev, double clip_eps, double vf_coef, double ent_coef,
                    float *dlogits_dev, float *dvalue_dev, float *dbias_actor_dev, float *dbias_critic_dev,
                    float *loss_dev, double *stats_dev, double *workspace_dev, void *stream);
/* merlin_ppo_loss plus grad_absmax_dev uint32[9] (or NULL): atomicMax of max over the frames of |dlogits[u][j]|
 * into [j] (j < act_dim) and of max |dvalue[u]| into [8], as float bits (the caller zeroes it) -- the bound
 * merlin_tower_head_bwd_planes derives dz's plane scale from. */
int merlin_ppo_loss_absmax(const float *logits_dev, const float *value_dev, const float *bias_actor_dev,
                           const float *bias_critic_dev, int64_t n_frames, int32_t act_dim, const int32_t *offs_dev,
                           const int32_t *order_dev, const int64_t *frame_of_dev, int64_t n_samples,
                           const int64_t *sample_index_dev, const int64_t *actions_dev, const float *logp_old_dev,
                           const float *adv_dev, const float *ret_dev, double clip_eps, double vf_coef,
                           double ent_coef, float *dlogits_dev, float *dvalue_dev, float *dbias_actor_dev,
                           float *dbias_critic_dev, float *loss_dev, double *stats_dev, double *workspace_dev,
                           uint32_t *grad_absmax_dev, void *stream);

/* Tower GEMM epilogues (csrc/merlin_head.hip): towers = 1 or 2, `rows` per tower; cols (hidden)
 * a multiple of 4 dividing 1024 (4 x a divisor of 256).  Column sums use a per-device library
 * workspace: calls on one device must be stream-ordered with each other.
 * bias_relu: z[t][r][c] = relu(z[t][r][c] + bias[t][c]) in place (NaN propagates), after a
 *            plain GEMM (conv3 / fc1 of CNNFeatureExtractor / the heads, actor_critic.py:9-41)
 * relu_bwd:  dz = [y > 0] * dy (dz may alias dy), dbias[t][c] = sum over r of dz[t][r][c]
 * head_bwd:  the heads' backward through fc1's ReLU (actor_critic.py:30-41): h float[2][n][hidden]
 *            = relu(fc1) of the actor / critic tower, dlogits float[n][act_dim], dvalue float[n],
 *            w_actor float[act_dim][hidden], w_critic float[hidden] ->
 *            dz[0][k] = [h0 > 0] * (dlogits[k] . w_actor), dz[1][k] = [h1 > 0] * dvalue[k] * w_critic,
 *            dbias float[2][hidden] = sum_k dz[t][k], dw_actor = dlogits^T h0, dw_critic = dvalue^T h1
 *            (fixed-order sums; act_dim <= 8); amax_dev (or NULL): atomicMax of max |dz| per tower as float
 *            bits into amax_dev[0..1] (zeroed by the caller; merlin_h3_gemm_*'s operand scale). */
int merlin_tower_bias_relu(float *z_dev, const float *bias_dev, int64_t rows, int32_t cols, int32_t towers,
                           void *stream);
int merlin_tower_relu_bwd(const float *y_dev, const float *dy_dev, float *dz_dev, int64_t rows, int32_t cols,
                          int32_t towers, float *dbias_dev, void *stream);
/* colsum: out float[towers][cols] = sum over r < rows of x[t * tower_stride + r * row_stride + c]
 * (fixed order; strides in floats, multiples of 4): the conv3 bias gradient from the per-window tap-0
 * rows of dQ (merlin/windows.py). */
int merlin_tower_colsum(const float *x_dev, int64_t rows, int32_t cols, int64_t row_stride, int64_t tower_stride,
                        int32_t towers, float *out_dev, void *stream);
int merlin_tower_head_bwd(const float *h_dev, const float *dlogits_dev, const float *dvalue_dev,
                          const float *w_actor_dev, const float *w_critic_dev, int64_t n, int32_t hidden,
                          int32_t act_dim, float *dz_dev, float *dbias_dev, float *dw_actor_dev,
                          float *dw_critic_dev, uint32_t *amax_dev, void *stream);
/* head_bwd_planes: head_bwd with dz written as its h3 planes dz_planes [2][n][hidden/8][2][8] f16 (merlin_h3_split's
 * layout, 4 B per value) instead of fp32, scaled by the power of two from a bound on max |dz| known before the pass:
 * dz_bound_dev[t] (written, float bits) = max over k of sum_j grad_absmax[j] |w_actor[j][k]| (tower 0) /
 * grad_absmax[8] |w_critic[k]| (tower 1), grad_absmax_dev from merlin_ppo_loss_absmax.  dz_bound_dev is then the
 * operand scale of the planes for merlin_h3_gemm_nt_planes / merlin_h3_gemm_tn_gather_planes_a.  hidden a multiple
 * of 8 dividing 1024. */
int merlin_tower_head_bwd_planes(const float *h_dev, const float *dlogits_dev, const float *dvalue_dev,
                                 const float *w_actor_dev, const float *w_critic_dev, int64_t n, int32_t hidden,
                                 int32_t act_dim, void *dz_planes_dev, float *dbias_dev, float *dw_actor_dev,
                                 float *dw_critic_dev, const uint32_t *grad_absmax_dev, uint32_t *dz_bound_dev,
                                 void *stream);
/* heads_fwd: the two heads (actor_critic.py:41-46, Linear(512, act_dim) / Linear(512, 1)) on h
 * float[2][n][hidden] = relu(fc1) of the actor / critic tower: logits float[n][act_dim] = h0 w_actor^T
 * (+ b_actor), value float[n] = h1 . w_critic (+ b_critic); biases may be NULL (not added).  hidden 512,
 * act_dim <= 8; one fixed summation order (every call the same bits). */
int merlin_tower_heads_fwd(const float *h_dev, int64_t n, int32_t hidden, const float *w_actor_dev,
                           int32_t act_dim, const float *w_critic_dev, const float *b_actor_dev,
                           const float *b_critic_dev, float *logits_dev, float *value_dev, void *stream);

/* fc1 (src/actor_critic.py:31-41, Linear(576, 512) of both towers) on the bf16 matrix cores in fp32
 * (csrc/merlin_gemm.hip): every fp32 operand value x is used as three bf16 planes x0 + x1 + x2 == x
 * (x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1)), and a product as the six plane products
 * with i + j <= 2 (the terms left out are below one fp32 rounding), summed per 32-deep k step and
 * added to the fp32 running sum once.  Replaces the three fp32 GEMMs of CNNActorCritic's fc1 in
 * PPO.update (forward src/actor_critic.py:40, backward through autograd at src/ppo.py:153-155).
 * The weights are passed as "x6 planes", bf16 [R][C/8][3][8] (per group of 8 values three 16-byte
 * chunks, planes 0, 1, 2; merlin_x6_split); the activations as plain fp32, split while staged.
 * split / join: n fp32 values (n % 8 == 0) <-> their planes (6 bytes per value).
 * gemm_nt:  C[t][m][n] = sum_k A[t][m][k] B[t][n][k], A fp32 [M][K], B planes [N][K] (K % 32 == 0;
 *           tower strides in values), + bias[t][n] and ReLU when bias != NULL; cfg selects the tile
 *           (0: 256x128, 1: 128x192, 2: 128x128, 3: 256x64; N a multiple of the tile width; 20..28 the
 *           32x32x16 MFMA kernels of csrc/merlin_gemm2.hip: 20 / 21 / 24 / 26 256x128, 22 / 23 / 27 128x192,
 *           25 / 28 128x128).  Any other cfg: MERLIN_E_UNSUPPORTED.
 * gemm_tn:  out[t][m][n] = sum_k A[t][k][m] B[t][k][n], A fp32 [Kd][M], B fp32 [Kd][N] (M, N multiples
 *           of the tile: cfg 0 / 2: 128x192, 1: 128x64; 20 / 21: 128x192 and 24 / 25: 256x192 on the
 *           32x32x16 MFMA), the k range cut into <= splits slabs
 *           (slab float[merlin_x6_tn_slab_floats(...)]) summed in slab order. */
int merlin_x6_split(const float *x_dev, int64_t n, void *planes_dev, void *stream);
int merlin_x6_join(const void *planes_dev, int64_t n, float *x_dev, void *stream);
int merlin_x6_gemm_nt(const float *A_dev, const void *B_dev, int64_t M, int32_t N, int32_t K, int32_t towers,
                      int64_t a_stride, int64_t b_stride, const float *bias_dev, float *C_dev, int64_t c_stride,
                      int32_t cfg, void *stream);
int64_t merlin_x6_tn_slab_floats(int32_t M, int32_t N, int32_t towers, int32_t splits);
int merlin_x6_gemm_tn(const float *A_dev, const float *B_dev, int64_t Kd, int32_t M, int32_t N, int32_t towers,
                      int64_t a_stride, int64_t b_stride, int32_t splits, float *slab_dev, float *out_dev, int32_t cfg,
                      void *stream);

/* fc1 (src/actor_critic.py:31-41) on the f16 matrix cores in fp32-class two-plane form (csrc/merlin_h3.hip, the
 * default of PPO.update's fc1 GEMMs): every operand x is scaled by a per-tower power of two 2^e (from its max |x|:
 * max |x| 2^e in [2^14, 2^15)) and used as two f16 planes h = f16(x'), l = f16((x' - h) 2^11); a product as the three
 * plane products h h, h l, l h (fp32 accumulation, the lo sum scaled by 2^-11 once), the result scaled back by
 * 2^-(eA + eB).  Error per output below the fp32 GEMM's (hipBLASLt) on the same operands (tests/test_gpu_h3.py).
 * Replaces the same three fp32 GEMMs as merlin_x6_* (forward src/actor_critic.py:40, backward src/ppo.py:153-155).
 * amax:  amax_dev[t] = float bits of max |x| over tower t's n values (x + t * stride; n, stride % 4 == 0); with n = 0
 *        it zeroes amax_dev[0 .. towers) (any count up to 2^20, by a kernel: safe inside a captured graph).
 * split: weight planes f16 [t][n/8][2][8] (per group of 8 values a hi and a lo 16-byte chunk), scaled by the
 *        exponent of amax_dev[t]; 4 bytes per value.
 * gemm_nt: C[t][m][n] = sum_k A[t][m][k] B[t][n][k], A fp32 [M][K] with its amax, B planes [N][K] (K % 32 == 0;
 *          tower strides in values), + bias[t][n] and ReLU when bias != NULL; cfg: 0 256x128, 1 128x192,
 *          2 128x128, 3 128x256, 5 128x64 (N a multiple of the tile width), 10..13 the same tiles as 0..3 with the
 *          split interleaved into the MFMAs (K >= 64), 14 the same at 64x128; 20 / 21 (256x128 / 128x192) both
 *          operands staged into LDS by DMA, 30 / 31 the same with the fragment reads under the MFMAs.  Any other cfg:
 *          MERLIN_E_UNSUPPORTED.  a_planes_dev (nullable; cfg < 20): receives A's planes as the kernel makes them
 *          ([t][M][K/8][2][8] f16, A's byte layout and tower stride) for a later gemm_tn_planes.
 * gemm_tn: out[t][m][n] = sum_k A[t][k][m] B[t][k][n], both fp32 with their amax (cfg 0 / 1: 128x192 tiles, M % 128,
 *          N % 192; 2: 64x192; 10 / 11: 0 / 1 with the split interleaved into the MFMAs), the k range cut into <= splits slabs (slab float[merlin_x6_tn_slab_floats(...)]) summed in slab
 *          order.
 * gemm_tn_planes: the same product over operands already in plane form (the a_planes output of gemm_nt for the same
 *          tensor and amax), strides in values.
 * gemm_nt_gather / gemm_tn_gather: gemm_nt (cfg 10..13) / gemm_tn (cfg 0..2) with the fp32 operand A / B read by
 *          64-value chunks through a row map: row r's chunk j (values 64 j .. 64 j + 63) is row rows_dev[r * K / 64 + j]
 *          (NT; TN: r * N / 64 + j) of the operand seen as [*][64] (tower stride as before; K or N % 64 == 0, K <= 576):
 *          conv3's rows through their patch representatives (merlin_tower_window_conv3_reuse with copy < 1). */
int merlin_h3_amax(const float *x_dev, int64_t n, int32_t towers, int64_t stride, uint32_t *amax_dev, void *stream);
int merlin_h3_split(const float *x_dev, int64_t n, int32_t towers, const uint32_t *amax_dev, void *planes_dev,
                    void *stream);
int merlin_h3_gemm_nt(const float *A_dev, const uint32_t *amax_a_dev, const void *B_dev, const uint32_t *amax_b_dev,
                      int64_t M, int32_t N, int32_t K, int32_t towers, int64_t a_stride, int64_t b_stride,
                      const float *bias_dev, float *C_dev, int64_t c_stride, void *a_planes_dev, int32_t cfg,
                      void *stream);
int merlin_h3_gemm_tn(const float *A_dev, const uint32_t *amax_a_dev, const float *B_dev, const uint32_t *amax_b_dev,
                      int64_t Kd, int32_t M, int32_t N, int32_t towers, int64_t a_stride, int64_t b_stride,
                      int32_t splits, float *slab_dev, float *out_dev, int32_t cfg, void *stream);
int merlin_h3_gemm_tn_planes(const void *A_planes_dev, const uint32_t *amax_a_dev, const void *B_planes_dev,
                             const uint32_t *amax_b_dev, int64_t Kd, int32_t M, int32_t N, int32_t towers,
                             int64_t a_stride, int64_t b_stride, int32_t splits, float *slab_dev, float *out_dev,
                             int32_t cfg, void *stream);
int merlin_h3_gemm_nt_gather(const float *A_dev, const uint32_t *amax_a_dev, const void *B_dev,
                             const uint32_t *amax_b_dev, int64_t M, int32_t N, int32_t K, int32_t towers,
                             int64_t a_stride, int64_t b_stride, const float *bias_dev, float *C_dev, int64_t c_stride,
                             const int32_t *a_rows_dev, int32_t cfg, void *stream);
/* gemm_nt_heads: the update's fc1 forward (both towers, bias + ReLU, cfg 10 / 12 / 13, a_rows_dev nullable as in
 *          gemm_nt_gather) with the policy / value heads (src/actor_critic.py:41-46) folded into the epilogue: per
 *          row, merlin_h3_heads_parts(N, cfg) partial dot products of h with head_w0 [n_actions][N] (tower 0, the
 *          actor; n_actions <= 4) and head_w1 [N] (tower 1, the critic), head_partials_dev float
 *          [2][parts][M][4]; merlin_heads_combine sums them in order: logits [M][n_actions], value [M] (no biases).
 *          C_dev may be NULL (towers' h not written; merlin_act_draw then finishes the acting step). */
int merlin_h3_gemm_nt_heads(const float *A_dev, const uint32_t *amax_a_dev, const void *B_dev,
                            const uint32_t *amax_b_dev, int64_t M, int32_t N, int32_t K, int64_t a_stride,
                            int64_t b_stride, const float *bias_dev, float *C_dev, int64_t c_stride,
                            const int32_t *a_rows_dev, const float *head_w0_dev, int32_t n_actions,
                            const float *head_w1_dev, float *head_partials_dev, int32_t cfg, void *stream);
int32_t merlin_h3_heads_parts(int32_t N, int32_t cfg);
/* h3_walk_blocks: the persistent plane-operand NT kernels (gemm_nt_planes cfg 62 / 78, gemm_nt_heads_planes cfg 60 /
 *          76: one block per CU walking a static list of tiles; 77 / 75 are the same kernels with a block per tile,
 *          the same bits) launch `blocks` blocks instead of one per CU until set back to 0.  Process-wide, for tests
 *          of the walk that must not depend on the device's CU count; never more blocks than tiles are launched. */
int merlin_h3_walk_blocks(int32_t blocks);
/* gemm_nt_planes: gemm_nt with A already in plane form too (A_planes [t][M][K/8][2][8] f16 scaled by amax_a_dev's
 *          exponent, e.g. merlin_tower_head_bwd_planes' dz), both operands staged into LDS by DMA (csrc/merlin_h3p.hip):
 *          cfg 60 128x256 / 62 128x192 tiles (62: the persistent kernel, a block per CU walking tiles, also 78; 77:
 *          the same tile with a block per tile, the same bits), K = 512 or 576, bias as gemm_nt.  Same products and order as gemm_nt
 *          on the fp32 A with the same scale: the same bits.  Measured alternates (round 6, not on the benched path):
 *          63 = 62 on a 4-stage ring; 66 = 62 with its MFMAs product-major (the same bits); 65 / 68 / 69 = one
 *          accumulator per tile (the lo planes rescaled in registers: another summation, held to float64 like the
 *          rest) on 256x192 / 256x256 (4 waves) / 192x192 tiles.
 * gemm_tn_gather_planes_a: gemm_tn_gather with A already in plane form (strides in values). */
int merlin_h3_gemm_nt_planes(const void *A_planes_dev, const uint32_t *amax_a_dev, const void *B_dev,
                             const uint32_t *amax_b_dev, int64_t M, int32_t N, int32_t K, int32_t towers,
                             int64_t a_stride, int64_t b_stride, const float *bias_dev, float *C_dev, int64_t c_stride,
                             int32_t cfg, void *stream);
/* gemm_nt_heads_planes: gemm_nt_heads (cfg 10 / 12 / 13, gathered rows, bias + ReLU, C_dev required) with A's
 *          gathered rows already h3 planes (merlin_tower_window_conv3_planes): staged as copies, no split; head_*
 *          NULL: h only.  With the planes of the same values and scale: gemm_nt_heads' bits.
 * gemm_tn_gather_planes: gemm_tn_gather with both operands as planes (dz from merlin_tower_head_bwd_planes, the
 *          gathered B from merlin_tower_window_conv3_planes). */
int merlin_h3_gemm_nt_heads_planes(const void *A_planes_dev, const uint32_t *amax_a_dev, const void *B_dev,
                                   const uint32_t *amax_b_dev, int64_t M, int32_t N, int32_t K, int64_t a_stride,
                                   int64_t b_stride, const float *bias_dev, float *C_dev, int64_t c_stride,
                                   const int32_t *a_rows_dev, const float *head_w0_dev, int32_t n_actions,
                                   const float *head_w1_dev, float *head_partials_dev, int32_t cfg, void *stream);
int merlin_h3_gemm_tn_gather_planes(const void *A_planes_dev, const uint32_t *amax_a_dev, const void *B_planes_dev,
                                    const uint32_t *amax_b_dev, int64_t Kd, int32_t M, int32_t N, int32_t towers,
                                    int64_t a_stride, int64_t b_stride, int32_t splits, float *slab_dev,
                                    float *out_dev, const int32_t *b_rows_dev, int32_t cfg, void *stream);
int merlin_h3_gemm_tn_gather_planes_a(const void *A_planes_dev, const uint32_t *amax_a_dev, const float *B_dev,
                                      const uint32_t *amax_b_dev, int64_t Kd, int32_t M, int32_t N, int32_t towers,
                                      int64_t a_stride, int64_t b_stride, int32_t splits, float *slab_dev,
                                      float *out_dev, const int32_t *b_rows_dev, int32_t cfg, void *stream);
/* The acting tail (merlin_act_heads' log-softmax, argmax or draw, action / logp / value) from the partials of a
 * merlin_h3_gemm_nt_heads call with C_dev = NULL (the acting path: h itself is never written), biases added here. */
int merlin_act_draw(const float *partials_dev, int32_t parts, int64_t n, const float *b_actor_dev,
                    const float *b_critic_dev, int32_t n_actions, int32_t deterministic, uint64_t seed,
                    const int64_t *epoch_dev, int64_t step, int64_t env_offset, int64_t *action_dev, float *logp_dev,
                    float *value_dev, void *stream);
int merlin_heads_combine(const float *partials_dev, int32_t parts, int64_t M, int32_t n_actions, float *logits_dev,
                         float *value_dev, void *stream);
int merlin_h3_gemm_tn_gather(const float *A_dev, const uint32_t *amax_a_dev, const float *B_dev,
                             const uint32_t *amax_b_dev, int64_t Kd, int32_t M, int32_t N, int32_t towers,
                             int64_t a_stride, int64_t b_stride, int32_t splits, float *slab_dev, float *out_dev,
                             const int32_t *b_rows_dev, int32_t cfg, void *stream);

/* The conv1 / conv2 tables of both towers and their adjoint (the parameter-only part of PPO.update's
 * minibatch step, merlin/fast_step.py WeightStage; replaces CNNActorCritic.conv2_tables and its autograd
 * backward, src/actor_critic.py:9-14 conv1 / conv2), csrc/merlin_stage.hip.  Per tower t < towers (1..2):
 * W1 f32[t][32][3][8][8], b1 f32[t][32], W2 f32[t][64][32][4][4] (the conv weights, towers stacked), atlas
 * f32[5][3][8][8] (the tile atlas / 255), idx int16[680][4] (the conv1-table entries of each tile
 * combination, CNNActorCritic._lut2_h1_index order).  Forward: HT f32[t][680][32] (relu(conv1) of every
 * combination, kept for the backward), T2 f32[t][2720][64].  Backward from dT2 f32[t][2720][64]: dH
 * f32[t][680][32] (scratch), dW1 / db1 / dW2 in the layouts of W1 / b1 / W2; koff int16[81] / kv int16[2720]
 * = the combinations v of each table entry k (CSR, (v, e) order).  Fixed-order sums (bitwise reproducible).
 * The backward keeps partial sums in a per-device library workspace: calls on one device run one at a time
 * (one stream, or ordered streams). */
/* The window GEMM's backward (Q = a2w W3r, conv3 per window; src/actor_critic.py:13 conv3 + the ReLU of conv2,
 * replacing CNNActorCritic's bmm / split-K bmm / relu backward in merlin/fast_step.py), csrc/merlin_winbwd.hip.
 * Per tower t < towers: a2w f32[t][nw][64] (relu(conv2) of the windows), dQ f32[t][nw][576], W3r f32[t][64][576] ->
 * da2w = [a2w > 0] * (dQ W3r^T) f32[t][nw][64], db2 = column sums of da2w f32[t][64], dW3r = a2w^T dQ
 * f32[t][64][576]; db3 (nullable) = column sums of dQ's first 64 columns f32[t][64] (tap 0: conv3's bias gradient).
 * exact-f32 MFMA products and sums, fixed order (bitwise reproducible).  work: scratch of at least
 * merlin_window_gemm_bwd_work(towers, nw) floats (-1: invalid arguments). */
int merlin_window_gemm_fwd(const float *a2w_dev, const float *W3r_dev, int32_t towers, int64_t nw, float *Q_dev,
                           void *stream);  /* Q = a2w W3r f32[t][nw][576], exact-f32 MFMA, fixed order */
int64_t merlin_window_gemm_bwd_work(int32_t towers, int64_t nw);
int merlin_window_gemm_bwd(const float *a2w_dev, const float *dQ_dev, const float *W3r_dev, int32_t towers, int64_t nw,
                           float *da2w_dev, float *db2_dev, float *dW3r_dev, float *db3_dev, float *work_dev,
                           int64_t work_floats, void *stream);
int merlin_stage_tables_fwd(const float *W1_dev, const float *b1_dev, const float *W2_dev, const float *atlas_dev,
                            const int16_t *idx_dev, int32_t towers, float *HT_dev, float *T2_dev, void *stream);
int merlin_stage_tables_bwd(const float *W2_dev, const float *HT_dev, const float *dT2_dev, const float *atlas_dev,
                            const int16_t *koff_dev, const int16_t *kv_dev, int32_t towers, float *dH_dev,
                            float *dW1_dev, float *db1_dev, float *dW2_dev, void *stream);
/* The weight-only chain of the optimizer step (merlin/fast_step.py NATIVE_CHAIN), same bits as the entry points above
 * with their torch neighbours:
 * merlin_stage_fwd_planes: merlin_stage_tables_fwd and, when x0_dev is given, merlin_h3_split of x0_dev / x1_dev
 *   (float [towers][n], n % 8 == 0) at the scale amax_dev[tower] into planes0_dev / planes1_dev, in one launch.
 * merlin_stage_bwd_scatter: merlin_stage_tables_bwd with dW1 / db1 / dW2 at offsets off_w1 / off_b1 / off_w2 of the
 *   derived-gradient buffer DG_dev, then flat_dev[map_dev[i]] = DG_dev[i] for i < n (map: distinct int32 indices
 *   into flat_dev) in the fold's launch: three launches.
 * merlin_gather_f32: dst_dev[i] = src_dev[map_dev[i]], i < n. */
int merlin_stage_fwd_planes(const float *W1_dev, const float *b1_dev, const float *W2_dev, const float *atlas_dev,
                            const int16_t *idx_dev, int32_t towers, float *HT_dev, float *T2_dev, const float *x0_dev,
                            const float *x1_dev, int64_t n, const uint32_t *amax_dev, void *planes0_dev,
                            void *planes1_dev, void *stream);
int merlin_stage_bwd_scatter(const float *W2_dev, const float *HT_dev, const float *dT2_dev, const float *atlas_dev,
                             const int16_t *koff_dev, const int16_t *kv_dev, int32_t towers, float *dH_dev,
                             float *DG_dev, int64_t off_w1, int64_t off_b1, int64_t off_w2, const int32_t *map_dev,
                             int64_t n, float *flat_dev, void *stream);
int merlin_gather_f32(const float *src_dev, const int32_t *map_dev, int64_t n, float *dst_dev, void *stream);

/* Optimizer step of PPO.update (src/ppo.py:153-156: clip_grad_norm_(params, max_norm) then
 * Adam.step(), replacing torch.nn.utils.clip_grad_norm_ + torch.optim.Adam(fused=True).step()) over
 * n_tensors (1..32) float32 parameter tensors, csrc/merlin_optim.hip.  params / grads / exp_avg /
 * exp_avg_sq / steps are host arrays of device pointers (steps: each tensor's Adam step counter,
 * float32[1], advanced by one), numel[i] > 0.  The gradients are scaled in place by
 * min(max_norm / (||g||_2 + 1e-6), 1) as clip_grad_norm_ does; norm_out (float32[1], NULL: not
 * written) gets ||g||_2 before clipping.  Adam: torch's fused arithmetic (no weight decay, amsgrad
 * or maximize).  workspace double[merlin_clip_adam_workspace(n_tensors, numel)]. */
int64_t merlin_clip_adam_workspace(int32_t n_tensors, const int64_t *numel);
int merlin_clip_adam(int32_t n_tensors, float *const *params, float *const *grads, float *const *exp_avg,
                     float *const *exp_avg_sq, float *const *steps, const int64_t *numel, double lr, double beta1,
                     double beta2, double eps, float max_norm, float *norm_out, double *workspace, void *stream);
/* merlin_clip_adam with its neighbours in the fast step's weight-only chain folded into the same two launches (the
 * parameters get the same bits).  Every params[i] lies in the flat buffer flat_dev[n_flat].  The first launch also
 * zeroes zero0_dev[n_zero0] and zero1_dev[n_zero1] (32-bit words, plain stores; NULL / 0: none).  The second also
 * writes each stepped value to its slots of the derived-weight buffer D_dev: slots_dev is int32 [n_flat][2], the (at
 * most two) indices into D_dev of each element of flat_dev, -1 = none.  For a tensor with amax_slot[i] >= 0 (host
 * array of n_tensors, NULL: none) it folds max |p| as float bits into amax_dev[amax_slot[i]] by atomicMax (the caller
 * has that word in a zero list).  total_dev (double[1], NULL: none) becomes total_dev[0] + (double)norm. */
int merlin_clip_adam_chain(int32_t n_tensors, float *const *params, float *const *grads, float *const *exp_avg,
                           float *const *exp_avg_sq, float *const *steps, const int64_t *numel, double lr, double beta1,
                           double beta2, double eps, float max_norm, float *norm_out, double *workspace,
                           uint32_t *zero0_dev, int32_t n_zero0, uint32_t *zero1_dev, int32_t n_zero1,
                           const float *flat_dev, int64_t n_flat, const int32_t *slots_dev, float *D_dev,
                           uint32_t *amax_dev, const int32_t *amax_slot, double *total_dev, void *stream);

/* Few-shot evaluation's inner step (src/distribution_over_tasks.py:200-203, src/fomaml.py:180-182:
 * clip_grad_norm_(fast.parameters(), max_norm) then SGD(lr).step()) for G independent parameter sets at once,
 * csrc/merlin_fewshot.hip, two launches.  params / grads are host arrays of n_tensors (1..32) device pointers,
 * tensor i float32[G][numel[i]] contiguous (task g's copy at g * numel[i]), numel[i] > 0.  Per task g:
 * norm = ||g's gradients||_2 (f64 sums, rounded to float), coef = min(max_norm / (norm + 1e-6), 1) with a NaN
 * kept, grads *= coef (written back, as clip_grad_norm_ does), params -= lr * grads.  Tasks never mix: a
 * non-finite gradient turns only its own task's parameters NaN.  No atomics: bitwise reproducible.  norm_out
 * float32[G] (NULL: not written) gets the pre-clip norms.  workspace
 * double[merlin_group_clip_sgd_workspace(n_tensors, numel, G)] (-1: bad arguments).  n_tensors = 0 or G = 0:
 * MERLIN_OK without a launch. */
int64_t merlin_group_clip_sgd_workspace(int32_t n_tensors, const int64_t *numel, int32_t G);
int merlin_group_clip_sgd(int32_t n_tensors, float *const *params, float *const *grads, const int64_t *numel,
                          int32_t G, float lr, float max_norm, float *norm_out, double *workspace, void *stream);

/* The per-episode loss of src/distribution_over_tasks.py:97-128 for n episodes stored [T][n] (row t, episode i at
 * t * n + i), episode i of length_dev[i] steps (int32, clamped to 1..T), one launch.  Over the episode's own steps
 * only: GAE backwards in merlin_gae's fp32 order with the bootstrap masked at the last step (the advantages,
 * written to workspace_dev float[T][n], equal merlin_gae's with done = 1 at the last step), mean and unbiased
 * standard deviation of the advantages (f64), adv_n = (adv - mean) / (std + 1e-8) (zeros for a 1-step episode),
 * ret = value + adv_n, loss_dev[i] = -mean(new_logp) + 0.5 * mean((new_value - ret)^2) (f64 sums).  Entries at
 * t >= length are neither read nor written. */
int merlin_episode_loss(const float *reward_dev, const float *value_dev, const float *new_logp_dev,
                        const float *new_value_dev, const int32_t *length_dev, int32_t T, int32_t n, double gamma,
                        double lam, float *workspace_dev, float *loss_dev, void *stream);

/* Finished episodes of a rollout by class: rows t*N+i with done_dev[row] != 0 contribute their ep_return / ep_length
 * to class class_dev[i] (< n_classes <= 8).  out_dev double[n_classes][4] = (episodes, sum return, sum return^2,
 * sum length); accumulate != 0 adds to out_dev instead of overwriting.  csrc/merlin_epstats.hip, two launches: fp64
 * sums in a fixed order, no atomics (two calls on the same input give the same bits), stream-ordered, no host
 * sync, no allocation (the per-block sums live in the library's per-device workspace, so two calls on one device
 * must be stream-ordered): safe inside a captured graph.  T = 0, N = 0 or a class with no finished episode: zeros
 * for that class.  An env whose class is >= n_classes is ignored. */
int merlin_episode_class_stats(const float *done_dev, const double *ep_return_dev, const int32_t *ep_length_dev,
                               const uint8_t *class_dev, int32_t T, int32_t N, int32_t n_classes,
                               double *out_dev, int32_t accumulate, void *stream);

/* ---- finite level sets and level replay ------------------------------------------------------------
 * Level mode: the context holds a bank of L maps and every map an env takes -- merlin_env_reset, the auto-reset of
 * every step kernel -- is a level of the bank instead of a generated map.  The k-th map env i takes since the bank
 * was bound is level l = the smallest index with u <= cdf[l], clamped to L - 1 (numpy searchsorted(cdf, u, 'left'),
 * clipped), u = the action draw's counter-keyed uniform in (0, 1] of (level_seed, epoch 0, step k, env env_offset + i,
 * j 0), compared in double: a pure function of (seed, global env index, k, the CDF in force at that reset), whichever
 * kernel resets.  Level mode reads and writes neither the envs' RNG streams nor their look-ahead maps (a reset never
 * raises MERLIN_DEVERR_SLOT_EMPTY, merlin_env_refill does nothing); everything after the map is taken is unchanged.
 *
 * merlin_env_set_levels: the bank in merlin_env_snapshot's layouts, device memory -- walls_dev uint32[L][size],
 * goal_dev int32[L][2], agent_dev int32[L][4] (x, y, dir, 0); coordinates are clamped into the grid, the maps'
 * validity is the caller's -- copied into context-owned buffers, with a uniform CDF (cdf[l] = (l + 1) / L), draw
 * counters 0 and current levels -1.  L = 0 or a null bank pointer unbinds level mode (the RNG streams and look-ahead
 * maps are as they were before it).  L outside 1..2^20: MERLIN_E_INVALID; a reseed_each_reset context:
 * MERLIN_E_UNSUPPORTED.  Allocates and synchronises the stream, like merlin_env_set_difficulties: not capturable, and a
 * graph captured under an earlier binding must be captured again. */
int merlin_env_set_levels(merlin_env *env, const uint32_t *walls_dev, const int32_t *goal_dev, const int32_t *agent_dev,
                          int64_t L, uint64_t level_seed, int64_t env_offset, void *stream);
/* cdf_dev double[L] (non-decreasing, last entry 1.0) copied into the bound CDF buffer in place, stream-ordered: a graph
 * captured earlier reads the new weights without a re-capture.  No allocation, no host sync: capturable. */
int merlin_env_set_level_cdf(merlin_env *env, const double *cdf_dev, void *stream);
/* cur_dev int32[num_envs] (the level each env is in; -1 before its first map), count_dev uint32[num_envs] (maps taken
 * since the bank was bound), either nullable.  One kernel: capturable. */
int merlin_env_levels(merlin_env *env, int32_t *cur_dev, uint32_t *count_dev, void *stream);
/* A context-bound log the step writes: every later merlin_env_step / merlin_env_act_step launch writes, for each of its
 * steps t, the level env i is in when it acts -- before the step and its auto-reset -- to log_dev[t * num_envs + i]
 * (int32[n_steps][num_envs]).  Host state read at launch, no launch of its own: a captured launch keeps the pointer it
 * was captured with.  NULL (and every new binding or unbinding of a bank): no log.  Before merlin_env_set_levels:
 * MERLIN_E_INVALID. */
int merlin_env_set_level_log(merlin_env *env, int32_t *log_dev);
/* [host] the draw restated on the CPU by the same lines the kernels run: out_host int32[n][k_count], entry (i, k) =
 * the level of draw k_first + k of global env env_first + i under cdf_host double[L]. */
int merlin_level_draw_host(uint64_t level_seed, int64_t env_first, int64_t n, int64_t k_first, int64_t k_count,
                           const double *cdf_host, int64_t L, int32_t *out_host);

/* Per-level scores of a rollout: step (t, i) with level_dev[t][i] in [0, L) adds llrint((double)f * 2^24), f =
 * fminf(kind == 0 ? fabsf(a) : fmaxf(a, 0), 32768.f), a = adv_dev[t][i] (the un-normalised GAE; kind 0 = the L1 value
 * loss, 1 = the positive value loss), to sum_dev[level] and 1 to count_dev[level]; other steps are skipped.  int64
 * sums: the result does not depend on the order of the additions.  accumulate = 0 zeroes both vectors first.
 * T * N > 2^24 (the sums' headroom), L outside 1..2^20, another kind or a null pointer: MERLIN_E_INVALID.  At most two
 * launches, 64-bit integer atomics after per-thread and per-block pre-reduction (csrc/merlin_levels.hip), no
 * allocation, no host sync: capturable. */
int merlin_level_scores(const float *adv_dev, const int32_t *level_dev, int32_t T, int32_t N, int64_t L, int32_t kind,
                        int64_t *sum_dev, int64_t *count_dev, int32_t accumulate, void *stream);
/* [host] the same sums on the CPU. */
int merlin_level_scores_host(const float *adv_host, const int32_t *level_host, int32_t T, int32_t N, int64_t L,
                             int32_t kind, int64_t *sum_host, int64_t *count_host, int32_t accumulate);

/* ---- level editing -----------------------------------------------------------------------------------
 * The edit rule.  A level is `size` = S wall rows, a goal (gx, gy) and an agent (x, y, dir), in merlin_env_snapshot's
 * layouts.  Child c of generation g is its parent after E edits applied in order e = 0 .. E - 1; edit e draws
 *   u_j  = the action draw's counter-keyed uniform in (0, 1] of (edit_seed, epoch g, step e, env c, j), j = 0, 1, 2
 *   kind = min((int)floor(u_0 * 4.0), 3)
 *   n    = min((int64)floor(u_1 * (double)((S-2)*(S-2))), (S-2)*(S-2) - 1)
 *   cell = (x, y) = (1 + n % (S-2), 1 + n / (S-2)): always an interior cell, the walled border is never touched
 *   kind 0, 1: toggle the wall bit at the cell; nothing if the cell is the agent's or the goal's
 *   kind 2:    the goal moves to the cell; nothing if it is a wall, the agent's cell or the goal's own
 *   kind 3:    the agent moves to the cell with dir = min((int)floor(u_2 * 4.0), 3); nothing if it is a wall or the
 *              goal's cell (the agent's own cell is allowed: a turn in place)
 * One double multiply and a floor per value: a restatement in another language is exact.  Per child the rule gives the
 * edited map, changed (uint8: 1 iff the walls, goal or agent differ from the parent's -- two toggles of one cell
 * cancel) and dist (int32: merlin_shortest_paths' value at the child's start pose, -1 if the goal cannot be reached).
 * A valid parent (border walled, agent and goal on distinct free cells) gives a valid child, possibly an unsolvable
 * one.
 *
 * merlin_levels_mutate: parents walls_dev uint32[P][size], goal_dev int32[P][2], agent_dev int32[P][4]; child c < C
 * edits parent parent_index_dev[c] (int32[C]; NULL: parent c, and then C <= P) into out_walls_dev uint32[C][size],
 * out_goal_dev int32[C][2], out_agent_dev int32[C][4], dist_dev int32[C], changed_dev uint8[C].  An index outside
 * [0, P) reads nothing: that child is all-zero rows, zero goal and agent, dist -1, changed 0.  edits = 0 copies the
 * parents (changed 0, dist the parents').  size outside 5..32, edits outside 0..64, a negative count or a null pointer
 * (parent_index_dev aside): MERLIN_E_INVALID; C = 0: nothing to do.  One kernel (csrc/merlin_level_edit.hip), no
 * allocation, no host sync: capturable. */
int merlin_levels_mutate(const uint32_t *walls_dev, const int32_t *goal_dev, const int32_t *agent_dev, int64_t P,
                         const int32_t *parent_index_dev, int64_t C, int32_t size, int32_t edits, uint64_t edit_seed,
                         uint64_t generation, uint32_t *out_walls_dev, int32_t *out_goal_dev, int32_t *out_agent_dev,
                         int32_t *dist_dev, uint8_t *changed_dev, void *stream);
/* [host] the same on host arrays in plain C++ (the search is merlin_shortest_paths_host's). */
int merlin_levels_mutate_host(const uint32_t *walls_host, const int32_t *goal_host, const int32_t *agent_host, int64_t P,
                              const int32_t *parent_index_host, int64_t C, int32_t size, int32_t edits,
                              uint64_t edit_seed, uint64_t generation, uint32_t *out_walls_host, int32_t *out_goal_host,
                              int32_t *out_agent_host, int32_t *dist_host, uint8_t *changed_host);
/* Child j < C (walls_dev uint32[C][size], goal_dev int32[C][2], agent_dev int32[C][4]) is packed into slot slot_dev[j]
 * (int32[C]) of the bound bank as merlin_env_set_levels packs it; a slot outside [0, L) skips its child (a rejected
 * child is dropped without a host read); distinct valid slots are the caller's to guarantee.  Stream-ordered and in
 * place: the bank's buffers keep their addresses, so a graph captured earlier plays the new maps without a re-capture.
 * The CDF, the draw counters and the envs' RNG are not touched.  An env that is inside a replaced slot keeps its own
 * copy of the old map to the end of its episode and its current level becomes -1: the step's level log writes -1 for
 * its remaining steps (merlin_level_scores skips them), so no step on the old map is credited to the new level.  No
 * allocation, no host sync: capturable.  Before merlin_env_set_levels: MERLIN_E_INVALID. */
int merlin_env_replace_levels(merlin_env *env, const int32_t *slot_dev, const uint32_t *walls_dev,
                              const int32_t *goal_dev, const int32_t *agent_dev, int64_t C, void *stream);
/* The bound bank copied out in merlin_env_snapshot's layouts: walls_dev uint32[L][size], goal_dev int32[L][2],
 * agent_dev int32[L][4], each nullable.  One kernel: capturable.  Before merlin_env_set_levels: MERLIN_E_INVALID. */
int merlin_env_level_bank(merlin_env *env, uint32_t *walls_dev, int32_t *goal_dev, int32_t *agent_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif
