/* shipenv.h — C-ABI of libshipenv_hip.so, the MI355X-native batched ShippingEnv step.
 *
 * The reference has no FFI: its "operator API" is the Python class
 * shipping.Environment (/root/reference/shipping/environment.py:28-376). Each
 * entry point below replaces one method of that class for N environments at
 * once; the Python mirror shippingenv_amd/shipping/environment.py binds them
 * through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - Every function returns 0 on success or a negative SE_E* status; the text of
 *    the last failure on the calling thread is se_last_error().
 *  - All N-sized buffers are DEVICE pointers owned by the caller (e.g. torch
 *    tensors' data_ptr()); the library never frees them. They must be 16-byte
 *    aligned. The library owns only its staged map/ports copies and scratch.
 *  - Launching calls take a hipStream_t as void* (NULL = the null stream), are
 *    asynchronous on it and never synchronise the host.
 *  - Per-environment failures are not API errors: they are reported per env in
 *    err[i] (SE_ERR_*), exactly where the reference raises an exception; such an
 *    env's state is left untouched with reward 0 and done 0.
 *  - n = 0 (an empty batch) is valid: the env's calls then launch nothing and accept
 *    null N-sized buffers; a step still advances the step counter.
 */
#ifndef SHIPENV_H
#define SHIPENV_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHIPENV_ABI_VERSION 2  /* 2: se_state.ep_start (episode-start stamps) replaces ep_len */

/* API status codes */
#define SE_OK 0
#define SE_EINVAL (-1)  /* bad argument */
#define SE_EHIP (-2)    /* HIP runtime error */
#define SE_ESTATE (-3)  /* call out of order (e.g. step before bind) */

/* Per-environment error classes; the Python mirror re-raises the reference's
 * exception type and message for each (shipping/environment.py line). */
#define SE_ERR_OK 0
#define SE_ERR_OOB 1            /* ValueError("Move is out of range")                       :284 */
#define SE_ERR_SAME_PORT 2      /* Exception("Destination port must be different ...")      :267 */
#define SE_ERR_PORT_RANGE 3     /* IndexError("Port index is out of range")                 :269 */
#define SE_ERR_NOT_AT_PORT 4    /* Exception("Not currently at port")                  :343, :352 */
#define SE_ERR_AMOUNT 5         /* ValueError("Invalid fuel amount")                   :346, :355 */
#define SE_ERR_NO_DEST 6        /* Exception("Cannot move without destination port")        :276 */
#define SE_ERR_BAD_CATEGORY 7   /* ValueError("Action category unknown")                    :374 */
#define SE_ERR_NO_PORTS 8       /* Exception("No ports available")                          :360 */
#define SE_ERR_BAD_INDEX 9      /* IndexError("list index out of range"), utils/preprocessing.py:127 */
#define SE_ERR_NEED_DRAW 10     /* replay only: the step needs a variate the tape lacks (no effect) */

/* se_tape.used bits written by se_step_replay: the reference draws the step consumed */
#define SE_USED_FUEL_GATE 1     /* uniform() for the fuel cost (:104) and the gate random() (:320) */
#define SE_USED_LOSS_TYPE 2     /* random() loss type (:177) */
#define SE_USED_BETA 4          /* betavariate(2, 2) (:195) */
#define SE_USED_ARRIVE 8        /* randint redraw of the destination (:333-335) */
#define SE_USED_MOVED 16        /* not a draw: the ship moved onto a non-ground cell (:296-300),
                                   so fuel became an np.float64 and the reward a float */

/* se_create flags */
#define SE_FLAG_AUTO_RESET 1u   /* reset an env inside se_step right after it reports done */

#define SE_NONE 255             /* origin/dest "None" in the u8 index fields */
#define SE_MAX_PORTS 254
#define SE_MAX_SIDE 256         /* H, W <= 256 (positions are u8) */
#define SE_MAX_CARGO 715827882  /* (2^31 - 1) / 3: |cargo| and |cargo + amount| stay within it (se_state.cargo) */

typedef struct se_env se_env;

/* Done-list entry written by the auto-reset path (wave-ballot compaction). */
typedef struct se_done_rec {
    int32_t env;         /* local env index */
    float ep_return;     /* return of the finished episode */
    int32_t ep_len;      /* its length in step calls */
    int32_t step;        /* the step counter value of the step that finished it */
} se_done_rec;

/* Per-env SoA state, one entry per environment, all device pointers (16-B aligned).
 * ep_return, ep_start, done_recs and done_count may be NULL unless SE_FLAG_AUTO_RESET.
 * Without that flag a step never writes them, bound or not; se_reset / se_reset_to write
 * ep_return and ep_start of the envs they reset whenever they are bound. No call writes outside
 * the documented entries of a buffer, before its first or past its last.
 * All calls on one env must be ordered on one stream (or externally synchronised):
 * the step kernel updates each wave's statistics-slab entry and the done lists with
 * plain loads and stores, which assumes no other launch on the same env overlaps it. */
typedef struct se_state {
    uint8_t* x;         /* ship_position[0], row of np_game      (environment.py:37,:241,:297) */
    uint8_t* y;         /* ship_position[1], column of np_game */
    double* fuel;       /* self.fuel, f64 like the reference (int 200 - sum of np.float64)  :39 */
    int32_t* cargo;     /* self.cargo                                                      :38
                           Contract: cargo, and cargo + amount of a TAKE_CARGO, stay within
                           +-SE_MAX_CARGO = (2^31 - 1) / 3, the largest value for which the
                           step's 3 * loss (and 2 * cargo at arrival) is exact in int32. The
                           reference's unbounded ints are matched only inside that range;
                           beyond it the int arithmetic wraps (shipping.Environment raises
                           OverflowError instead). Negative cargo is inside the contract. */
    uint8_t* origin;    /* self.origin_port_index, SE_NONE = None                          :40 */
    uint8_t* dest;      /* self.destination_port_index, SE_NONE = None                     :41 */
    float* reward;      /* step() reward, the reference's f64 value rounded once to f32    :376 */
    uint8_t* done;      /* step() done                                                     :376 */
    int8_t* err;        /* SE_ERR_* per env */
    float* ep_return;   /* running episode return (auto-reset) */
    int32_t* ep_start;  /* auto-reset: the step-counter value (mod 2^32) at which the env's
                           current episode began; its running length in step calls is
                           (step counter - ep_start) mod 2^32. A step writes it only for
                           the envs it resets (about 1 in 240 per step), where a running
                           length was read and written for every env on every step.
                           se_reset / se_reset_to stamp the counter's current value; a
                           checkpoint restores it together with se_set_counters. */
    struct se_done_rec* done_recs; /* auto-reset done lists: 2 * segments * seg_stride records
                                      (se_done_layout), double-buffered by step parity */
    int32_t* done_count;           /* auto-reset per-segment counts: 2 * segments entries. se_bind
                                      (auto-reset) and se_set_counters (whenever it is bound) clear
                                      them with a synchronous memset; a step writes all `segments`
                                      counts of its parity half and nothing of the other half */
    double* reward64;              /* optional (NULL): the reference's f64 reward, unrounded */
} se_state;

/* One replayed MOVE's variates (the draws the reference made through `random`,
 * SURVEY.md Appendix A); used by se_step_replay only. 40 bytes, no padding; the replaying
 * calls read the first 36 and write `used` alone. A variate the
 * step needs but the record lacks (NaN, or arrive_dest < 0) yields
 * SE_ERR_NEED_DRAW and no state change: a caller holding the reference's RNG
 * draws exactly that next variate and steps again (shipping.Environment does). */
typedef struct se_tape {
    double u_fuel;       /* random() behind uniform(-0.1, 0.1)                  :104 */
    double u_gate;       /* random() of the cargo-loss gate                       :320 */
    double u_type;       /* random() loss type (read only if the gate fires)      :177 */
    double beta;         /* betavariate(2, 2) (read only for a partial loss)      :195 */
    int32_t arrive_dest; /* accepted randint at arrival                          :333 */
    int32_t used;        /* out: SE_USED_* bits of the draws the step consumed */
} se_tape;

/* Environment.__init__ + _initialize_map + add_port (environment.py:29-65).
 * water: H*W bytes row-major [x*W + y], 0 = GROUND, nonzero = not ground (the
 * thresholded map of :45-55). Ports are stamped non-ground like add_port (:65).
 * port_fuel / port_cargo: the stocks add_port drew (:63-64). P may be 0.
 * env_id_base: global id of env 0 (rank * n for sharded runs): the Philox key
 * (seed, env_id_base + i) makes results shard-invariant. */
int se_create(se_env** out, int device, int64_t n, int64_t env_id_base, int32_t H, int32_t W,
              const uint8_t* water, int32_t P, const int32_t* port_x, const int32_t* port_y,
              const int32_t* port_fuel, const int32_t* port_cargo, uint64_t seed, uint32_t flags);

/* Replace the ports table (add_port / remove_port / attribute assignment); host arrays. */
int se_set_ports(se_env* env, int32_t P, const int32_t* port_x, const int32_t* port_y,
                 const int32_t* port_fuel, const int32_t* port_cargo);

/* Bind the caller-owned SoA buffers (n entries each, 16-byte aligned): device memory,
 * or pinned host memory, which ROCm maps into the GPU's address space (the N = 1
 * shipping.Environment binds one pinned 256-byte block and reads results in place). */
int se_bind(se_env* env, const se_state* state);

/* reset() (environment.py:227-243) for every env with mask[i] != 0 (mask NULL = all):
 * cargo 0, fuel 200, origin ~ U{0..P-1}, dest ~ U{others}, ship at the origin port; reward,
 * done, err and ep_return 0, ep_start the step counter. An env with mask[i] == 0 keeps every
 * byte of every field, reward, done and err included; the done lists are not touched.
 * Draws: Philox(seed, env) at counter (reset epoch, slot 5); the epoch advances per call. */
int se_reset(se_env* env, const uint8_t* mask, void* stream);

/* reset() with given origin/dest per env (device int32 arrays): replays a
 * recorded reset, or restores a state. */
int se_reset_to(se_env* env, const uint8_t* mask, const int32_t* origin, const int32_t* dest,
                void* stream);

/* step() for all envs with actions in the agent-index encoding of
 * utils/preprocessing.py:111-137 (a < 4 move N,E,S,W; < 4+P select; < 4+P+50
 * take cargo; else take fuel). Draws from Philox(seed, env) at counter
 * (step counter, slot); the step counter advances by one per call. */
int se_step(se_env* env, const int32_t* actions, void* stream);

/* `steps` consecutive steps issued from native code: step k takes its actions from
 * actions + k * ld (ld >= n int32 entries, 16-byte aligned rows; the ld - n entries behind a
 * row's n are neither read nor written), for a fixed action
 * schedule (a rollout of a pre-computed policy, the bench's timed region).
 * Guaranteed: the final state (x, y, fuel, cargo, origin, dest), the last step's reward, done
 * and err, and the step counter equal `steps` se_step calls on the same rows, bit for bit.
 * Without auto-reset the run is fused: the state of an env stays in registers from step
 * to step (step_seq_kernel; one launch per run of at most SHIPENV_SEQ_MAX_STEPS steps,
 * default 1024, read at se_create), so the intermediate steps' reward, done and err are
 * NOT written: the buffers hold the last step's alone, as the state buffers hold only
 * the final state. The steps of a launch before its last do not compute reward, done or
 * err at all, only the state (the last step of every launch is a full one).
 * In a fused launch's state-only steps a wave draws the cargo-loss gate's Philox block only for
 * its lanes that carry cargo, ahead of time and into wave-private LDS (6 KiB per workgroup
 * behind the world image and the 2 KiB table of stocks by cell code); SHIPENV_SEQ_GATE_POOL=0
 * at se_create, or a world image that leaves no room for it under the 64 KiB of a launch,
 * draws it for every lane every step instead. The results are the same bits.
 * A wave all of whose envs are inside the map and have a destination steps on a copy of the cell
 * codes with a border of one cell around the map (LDS behind the pools; 10.2 KiB for a 100 x 100
 * map): a move off the map reads the border's code, so such a step has no bounds test. On maps
 * up to 125 cells wide such a wave carries each ship's position as its cell's address in that
 * copy, and a move adds a byte from four per-direction deltas kept behind it (16 bytes). Worlds
 * of more than 253 ports, worlds whose table would leave fewer than four workgroups on a compute
 * unit, and every world under SHIPENV_SEQ_RING=0 at se_create have no such table; their waves,
 * and any wave with an env loaded outside the map or without a destination, run the general
 * step. The results are the same bits.
 * SHIPENV_SEQ_FUSE=0 at se_create issues one se_step launch per step
 * instead (the same kernel code as se_step's under a trace name of its own). With
 * auto-reset the run is always a launch per step (done lists, statistics and episode
 * counters are per step). An extension: the reference steps one call at a time
 * (environment.py:359-376). */
int se_step_seq(se_env* env, const int32_t* actions, int64_t ld, int32_t steps, void* stream);

/* se_step_seq that also records `event` (a hipEvent_t, may be NULL) on the stream right
 * after step number `mark_after` (0..steps; 0 = before the first launch): a timer mark
 * in the same native call as the launches, with no host round trip between them
 * (tools/diag/wall_forms.py). A fused run is split there: steps [0, mark_after), the
 * event, steps [mark_after, steps). */
int se_step_seq_mark(se_env* env, const int32_t* actions, int64_t ld, int32_t steps, void* stream,
                     void* event, int32_t mark_after);

/* step() with the reference's typed action [ActionType, value] (environment.py:359-376):
 * type 1..4 (shipping/type.py:1-5); MOVE value = (a, b) any integers; others value = a. */
int se_step_typed(se_env* env, const int32_t* type, const int32_t* a, const int32_t* b,
                  void* stream);

/* step() with typed actions whose variates come from tape[i] (replay of recorded
 * reference draws); writes tape[i].used. The step counter does not advance. */
int se_step_replay(se_env* env, const int32_t* type, const int32_t* a, const int32_t* b,
                   se_tape* tape, void* stream);

/* step() for agent-index actions (the se_step encoding) with the reference's draws from
 * tape[i] instead of Philox: the production step kernel's own code path (the agent path
 * se_step runs) in its replay-tape instantiation, for parity against the reference's
 * records. Writes tape[i].used; a step that needs a variate tape[i] lacks answers
 * SE_ERR_NEED_DRAW with no effect. The step counter does not advance. */
int se_step_agent_replay(se_env* env, const int32_t* actions, se_tape* tape, void* stream);

/* The N = 1 GPU stepper as one resident wave (csrc/server.h): se_step_replay / se_reset_to
 * on a one-env handle without a launch or a stream synchronise per call. The env's state,
 * typed action and tape and the mailbox are one se_server_block in coherent pinned host memory
 * (se_host_alloc, 64-byte aligned); the caller writes a call's inputs there, se_server_call
 * posts the op and returns when the wave has answered, the outputs then in the same block:
 *   SE_SERVER_STEP      se_step_replay (environment.py:359-376): x .. b and tape in, state,
 *                       reward, reward64, done, err and tape.used out
 *   SE_SERVER_RESET_TO  se_reset_to with origin = type, dest = a (:227-243); they must name
 *                       ports (not checked on the device)
 * The wave ends after 20 ms without a call and is launched again by the next one;
 * se_server_destroy ends it (destroy the server before its env). The handle may also be
 * bound (se_bind) to the block's fields for the launch path (se_step_replay). An extension:
 * the reference steps in Python (Environment.step). */
#define SE_SERVER_STEP 1
#define SE_SERVER_RESET_TO 2
typedef struct se_server_block {
    uint8_t x, y, origin, dest, done;  /* 0 (origin / dest SE_NONE = None) */
    int8_t err;
    uint8_t pad0[2];
    double fuel;                       /* 8 */
    int32_t cargo;                     /* 16 */
    float reward;                      /* 20 */
    double reward64;                   /* 24 */
    int32_t type, a, b;                /* 32 */
    uint32_t seq0;                     /* 44: se_server_call: the call's number, line 0's copy */
    se_tape tape;                      /* 48 */
    uint32_t seq1;                     /* 88: the call's number again, stored last */
    uint32_t op;                       /* 92 */
    uint32_t answer;                   /* 96: the wave: the number of the call it answered */
    uint32_t running;                  /* 100: the wave: 0 once it has ended */
    uint8_t pad1[24];
} se_server_block;                     /* 128 bytes: two 64-byte lines */
typedef struct se_server se_server;
int se_host_alloc(size_t bytes, void** out);  /* zeroed, coherent, device-mapped, 64-byte aligned */
int se_host_free(void* p);
int se_server_create(se_server** out, se_env* env, se_server_block* block);
int se_server_call(se_server* s, int32_t op);
int se_server_launches(se_server* s, uint64_t* out);  /* kernel launches so far (idle restarts + 1) */
int se_server_destroy(se_server* s);

/* Host-resident environments (no device, no HIP call): the N = 1 drop-in
 * shipping.Environment steps here by default (shippingenv_amd/shipping/_host.py), with the
 * step kernels' own per-env code compiled for the host (replay_env in env_core.h), so a
 * reference step() costs one C call instead of a kernel launch and a stream synchronise.
 * The state buffers are host memory; no alignment is required.
 *   se_host_create / se_host_set_ports   Environment.__init__ + add_port (:29-65)
 *   se_host_step_replay                  step() (:359-376) with the reference's draws from
 *                                        tape[i], exactly as se_step_replay
 *   se_host_reset_to                     reset() (:227-243) to given origin / dest
 */
typedef struct se_host se_host;
int se_host_create(se_host** out, int32_t H, int32_t W, const uint8_t* water, int32_t P,
                   const int32_t* port_x, const int32_t* port_y, const int32_t* port_fuel,
                   const int32_t* port_cargo);
int se_host_set_ports(se_host* h, int32_t P, const int32_t* port_x, const int32_t* port_y,
                      const int32_t* port_fuel, const int32_t* port_cargo);
int se_host_step_replay(se_host* h, int64_t n, const se_state* st, const int32_t* type,
                        const int32_t* a, const int32_t* b, se_tape* tape);
/* se_host_reset_to stamps ep_start = 0 (a host world keeps no step counter): lengths derived
 * from a host world's stamps (counter - ep_start) are meaningless; the host stepper reports
 * lengths through its own step records. */
int se_host_reset_to(se_host* h, int64_t n, const se_state* st, const uint8_t* mask,
                     const int32_t* origin, const int32_t* dest);
int se_host_destroy(se_host* h);

/* utils.preprocessing.preprocess_state rows (:25-62) as f32, n rows of 6+4P entries at row
 * stride ld >= 6+4P (the ld - (6+4P) entries behind a row are not written; the state is only read):
 * [x, y, fuel, fuel ("cargo" is self.fuel, environment.py:206), origin, dest, (px,py,pfuel,pcargo)*P],
 * None -> -1. */
int se_observe(se_env* env, float* obs, int64_t ld, void* stream);

/* DQN is_valid_action (agents/dqn.py:125-175) for every agent index a < 4+P+250,
 * packed MSB-first per row (numpy.packbits order), row stride ceil((4+P+250)/8) bytes. */
int se_valid_mask(se_env* env, uint8_t* bits, void* stream);

/* Synthetic agent: fills actions[i] (n entries; the state is neither read nor written) from
 * Philox(seed, env) at (t, slot 6) with the
 * bench mix (90% move, 5% take cargo U{1..20}, 3% take fuel U{1..20}, 2% select). */
int se_gen_actions(se_env* env, int32_t* actions, uint32_t t, void* stream);

/* sample_action() (environment.py:245-263), the random policy of MCTS rollouts and
 * SARSA exploration, for every env from its current state, as typed actions (the
 * input of se_step_typed). One draw per env: Philox(seed, env) at (t, slot 11) word 0.
 *   at a port with no destination: SELECT_PORT uniform over the other ports   :247-253
 *   at a port with cargo 0:        TAKE_CARGO U{1..port_cargo} (randint :160)  :255-257
 *   at a port with fuel == 0:      the reference raises TypeError (self.fuel[idx], :163)
 *   otherwise:                     MOVE_SHIP N/E/S/W uniform (random.choice :165-167)
 * Where the reference raises (the fuel branch; randint(1, 0) on an empty port) the
 * type is SE_SAMPLE_RAISES; where it never returns (no other port, :253) it is
 * SE_SAMPLE_NO_OTHER_PORT. */
#define SE_SAMPLE_RAISES (-1)
#define SE_SAMPLE_NO_OTHER_PORT (-2)
int se_sample_actions(se_env* env, int32_t* type, int32_t* a, int32_t* b, uint32_t t, void* stream);

/* MCTS random rollouts (agents/mcts.py:211-238): rollout r starts from a copy of env
 * src[r]'s state (env state is not modified) and repeats sample_action + step until
 * the step reports done, max_steps steps have counted, or max_attempts attempts
 * have run. An attempt whose step raises is retried without counting (the
 * reference's `except Exception: continue`). Outputs (device, m entries):
 * ret[r] = the step rewards summed in f64 in order (total_reward, :226-230);
 * steps[r] = counted steps; status[r] = SE_ROLL_*.
 * Draws: Philox(seed, rollout_base + r) at (attempt, slot 12): sample word, u_fuel,
 * u_gate, u_type; and, for a partial loss or an arrival, (attempt, slot 13): three
 * beta uniforms, the new destination. */
#define SE_ROLL_DONE 0        /* the last counted step reported done */
#define SE_ROLL_MAX_STEPS 1   /* max_steps steps counted */
#define SE_ROLL_RAISED 2      /* sample_action raised; the exception leaves _rollout */
#define SE_ROLL_ATTEMPTS 3    /* max_attempts reached (the reference keeps retrying) */
#define SE_ROLL_BAD_SRC 4     /* src[r] outside [0, n) */
int se_rollout(se_env* env, const int32_t* src, int64_t m, int32_t max_steps, int32_t max_attempts,
               int64_t rollout_base, double* ret, int32_t* steps, int32_t* status, void* stream);

/* Scripted rollouts: what happens to env src[r] if it plays this action sequence, without
 * playing it. Rollout r starts from a copy of env src[r]'s state (the env's state and counters
 * are not modified) and plays its plan, position k = 0 .. len - 1 in turn:
 *   - a step that raises (err != SE_ERR_OK) leaves the copy untouched, adds no reward, is not
 *     counted and adds 1 to raised (se_rollout's `except Exception: continue`); the plan goes on;
 *   - any other step adds its f64 reward to ret[r] in order and 1 to counted[r]; if it reports
 *     done the rollout ends there with SE_PLAN_DONE and the rest of the plan is not played.
 * Plans are step-major: the action of position k of rollout r is element k * ld + r, ld >= m,
 * rows 16-byte aligned (the arrays, and ld a multiple of 4 when steps > 1). Two encodings:
 *   typed        type, a, b as se_step_typed takes them; a type outside 1..4 raises
 *                SE_ERR_BAD_CATEGORY as there, so type 0 pads a plan;
 *   agent index  a == b == NULL and type holds agent indices as se_step takes them; an index
 *                below -4 raises SE_ERR_BAD_INDEX as there.
 * len (NULL: steps for every rollout) gives each rollout's plan length, clamped to [0, steps].
 * Outputs (device, m entries): ret, counted, status = SE_PLAN_*, and what `out` asks for.
 * Draws: Philox(seed, id) with id = ids ? ids[r] : rollout_base + r (equal ids give common
 * random numbers). Position k reads (k, slot 12) words 1-3: u_fuel, u_gate, u_type; and, for a
 * partial loss or an arrival, (k, slot 13): three beta uniforms, the new destination. Word 0 of
 * slot 12, se_rollout's sample word, is not read. The counter is the plan position, raising
 * steps included, so these are the draws of attempt k of se_rollout's rollout with the same id:
 * a scripted rollout whose plan is that rollout's attempt list equals it in ret (bits), steps,
 * done-ness and the final ship.
 * Misuse (a null required buffer with m > 0, ld < m, a negative m, steps or rollout_base, one
 * of a / b NULL, misaligned rows) is SE_EINVAL before any launch; m = 0 is a no-op; steps = 0
 * writes ret 0, counted 0 and SE_PLAN_END. The call allocates nothing and does not synchronise:
 * it may be captured into a graph. */
#define SE_PLAN_DONE 0     /* a counted step reported done; later actions not played */
#define SE_PLAN_END 1      /* the plan ran out */
#define SE_PLAN_BAD_SRC 4  /* src[r] outside [0, n): ret 0, steps 0, nothing else written but zeros/-1 */
typedef struct se_plan_out {   /* every pointer may be NULL: not wanted; m entries each */
    int32_t *raised, *first_err, *first_err_at;   /* count; SE_ERR_* of the first raising step (0) and its position (-1) */
    int32_t *x, *y; double *fuel; int32_t *cargo, *origin, *dest;  /* the ship when the rollout ended, -1 = None;
                                                                      a bad source: fuel 0, the others -1 */
} se_plan_out;
int se_rollout_plan(se_env* env, const int32_t* src, int64_t m,
                    const int32_t* type, const int32_t* a, const int32_t* b,  /* a == b == NULL: type holds agent indices */
                    int64_t ld, int32_t steps, const int32_t* len /* NULL: steps; else clamped to [0, steps] */,
                    const int64_t* ids /* NULL: rollout_base + r */, int64_t rollout_base,
                    double* ret, int32_t* counted, int32_t* status, const se_plan_out* out, void* stream);

/* The navigator (an extension: the reference has no such component): route tables for the env's
 * static world, an expert policy that reads them, and rollouts that play it.
 *
 * Tables, built on the host by one breadth-first pass per port from the water mask and the ports
 * as se_create sees them (ports stamped non-ground, x the row), cell c = x * W + y:
 *   field[p][c]  u16: the least number of moves from c to port p's cell, every cell of the path
 *                in the map and not ground; 0 on the port's cell, SE_NAV_INF on ground and where
 *                there is no such path (no finite value reaches SE_NAV_INF for H, W <= 256).
 *   dir[p][c]    u8: the move k of the in-map neighbour with the smallest finite field[p] value,
 *                k = 0..3 = N (0,-1), E (-1,0), S (0,1), W (1,0) on (x, y) as in the agent index;
 *                the lowest k wins a tie; SE_NAV_NONE when no neighbour is finite (an enclosed
 *                cell, a 1 x 1 map). On the port's own cell it names a neighbour with field 1:
 *                step off and come back, since the step tests for an arrival only inside a move.
 * se_nav_build_host uses no device. Its checks are se_create's (sides 1..256, P 0..254, ports in
 * the map); P = 0 is a no-op; field and dir hold P * H * W entries each, either may be NULL.
 *
 * The policy, on a ship (x, y, fuel, cargo, origin, dest) with cur the port on its cell (the
 * first one there) or none, the first rule that applies:
 *   1. dest None: at sea SE_NAV_NO_DEST; on a port SELECT_PORT q, the port q != origin with the
 *      smallest field[q][c] in 0 < field < SE_NAV_INF, the lowest q on a tie; none: SE_NAV_NO_DEST.
 *   2. on a port, fuel < refuel_below and its fuel stock >= 1: TAKE_FUEL of the whole stock.
 *   3. on a port, cargo == 0, load > 0 and its cargo stock >= 1: TAKE_CARGO min(load, stock).
 *   4. k = dir[dest][c]: SE_NAV_NONE is SE_NAV_UNREACHABLE, else MOVE_SHIP by move k.
 * A ship outside the map, or with a dest that names no port, is SE_NAV_UNREACHABLE: no table index
 * is formed from such a value, nor from a dir byte of SE_NAV_NONE. On any status but SE_NAV_OK the
 * action is (0, 0, 0), which se_step_typed answers with SE_ERR_BAD_CATEGORY and an untouched env.
 * No emitted action raises in the step: moves go to in-map non-ground cells, takes are within
 * stock, the selected port is not the origin. refuel_below compares as a double does (NaN never
 * refuels, +inf always); load < 0 is SE_EINVAL.
 *
 * The handle holds the tables for the env's current world on the host and the device. Destroy it
 * before its env. After se_set_ports every call but se_nav_rebuild and se_nav_destroy answers
 * SE_ESTATE ("the ports changed since se_nav_create: call se_nav_rebuild") and launches nothing;
 * se_nav_rebuild synchronises the device and is not capturable. P = 0 is a valid handle: its
 * calls report every env as SE_NAV_NO_DEST or SE_NAV_UNREACHABLE. max_leg is the largest finite
 * field value between two ports' cells, 0 if there is none. */
#define SE_NAV_INF 0xFFFF
#define SE_NAV_NONE 255
#define SE_NAV_OK 0
#define SE_NAV_NO_DEST 1
#define SE_NAV_UNREACHABLE 2
int se_nav_build_host(int32_t H, int32_t W, const uint8_t* water, int32_t P,
                      const int32_t* port_x, const int32_t* port_y,
                      uint16_t* field /* P*H*W or NULL */, uint8_t* dir /* P*H*W or NULL */);
typedef struct se_nav se_nav;
int se_nav_create(se_nav** out, se_env* env);
int se_nav_rebuild(se_nav* nav);
int se_nav_tables(const se_nav* nav, const uint16_t** d_field, const uint8_t** d_dir, int32_t* max_leg);
int se_nav_destroy(se_nav* nav);

/* The policy's action for every env of the handle's env (n entries each, 16-byte aligned; the
 * env's state is only read, nothing is drawn): type, a, b as se_step_typed takes them, status =
 * SE_NAV_*; agent (NULL: not wanted) the se_step index of the action, -1 where status != SE_NAV_OK
 * or the amount has no index (the index decodes to TAKE_CARGO 0..49 and TAKE_FUEL 0..199); dist
 * (NULL: not wanted) field[dest][cell], -1 for dest None, a dest that names no port, a ship outside
 * the map or SE_NAV_INF. A negative load or a misaligned array is SE_EINVAL whatever the handle;
 * n = 0 is a no-op. One launch, no allocation, no synchronisation: capturable. */
int se_nav_actions(se_nav* nav, double refuel_below, int32_t load,
                   int32_t* type, int32_t* a, int32_t* b, int32_t* status,
                   int32_t* agent, int32_t* dist, void* stream);

/* Navigated rollouts: se_rollout_plan's loop with the action of every position computed by the
 * policy from the rollout's private ship. Rollout r copies env src[r] (the env's state and
 * counters are only read) and plays positions k = 0 .. steps - 1: a raising step is skipped and
 * counted in end.raised (by the policy's construction there is none); a counted step adds its f64
 * reward in order, and one that reports done ends the rollout with SE_PLAN_DONE; a position where
 * the policy has no action ends it with SE_PLAN_STUCK, stuck_at = k and nav_status the SE_NAV_*
 * reason, and nothing more is played; running out of positions is SE_PLAN_END. arrivals counts the
 * steps that arrived at their destination. nav_status is SE_NAV_OK and stuck_at -1 otherwise.
 * Draws: no new slot. Key (seed, ids ? ids[r] : rollout_base + r); position k reads (k, slot 12)
 * words 1-3 and (k, slot 13) for a partial loss or an arrival: exactly se_rollout_plan's reads.
 * A navigated rollout equals se_rollout_plan on the same source and id, fed the action list the
 * navigator emitted, in ret (bits), counted, raised, done-ness and the end ship.
 * Misuse (a null required buffer with m > 0, a negative m, steps, rollout_base or load, a
 * misaligned array) is SE_EINVAL before any launch and whatever the handle; m = 0 is a no-op;
 * steps = 0 writes ret 0, counted 0 and SE_PLAN_END; a bad src[r] writes SE_PLAN_BAD_SRC with the
 * zeros and -1 se_rollout_plan writes. One launch, no allocation, no synchronisation: capturable. */
#define SE_PLAN_STUCK 5   /* the navigator had no action at some position; nav_status says which */
typedef struct se_nav_out {   /* every pointer may be NULL: not wanted; m entries each */
    int32_t *arrivals, *nav_status, *stuck_at;
    se_plan_out end;
} se_nav_out;
int se_rollout_nav(se_nav* nav, const int32_t* src, int64_t m, int32_t steps,
                   double refuel_below, int32_t load,
                   const int64_t* ids /* NULL: rollout_base + r */, int64_t rollout_base,
                   double* ret, int32_t* counted, int32_t* status, const se_nav_out* out, void* stream);

/* One MCTS decision per env (agents/mcts.py:240-292, MCTSAgent.choose_action): `simulations`
 * sequential simulations (UCB1 selection with c_param, one expansion, a random rollout of at
 * most max_rollout_steps counted steps, backpropagation) on a private copy of the env, whose
 * state is not modified, then best_child(c_param=0) over the root's children, or
 * sample_action() when the root has none. Outputs (device, n entries, 16-byte aligned): the
 * chosen typed action (type, a, b: se_step_typed's input) and status = SE_MCTS_*. tree and
 * tree_count (both or neither; NULL: not wanted) receive every node of env i in creation
 * order at tree[i * (simulations + 1) + j], j < tree_count[i], node 0 the root (parent -1,
 * no action); entries from tree_count[i] on are not written.
 * Draws: simulation s of env i uses Philox(seed, id), id = mcts_base + (env_id_base + i) *
 * simulations + s (a per-rollout key like se_rollout's). Tree step d of the simulation (the
 * selection steps, then the expansion step, d from 0) reads (d, slot 18): word 0 picks among
 * the untried actions (the expansion step alone reads it), words 1-3 are u_fuel, u_gate,
 * u_type; and, for a partial loss or an arrival, (d, slot 19): three beta uniforms, the new
 * destination. The simulation's rollout draws what se_rollout draws for rollout_base + r = id.
 * The root fallback reads word 0 of (0xFFFFFFFF, slot 18) of simulation 0's key.
 * np.log(parent.visits) is read from a table the library fills with the host's log(). */
#define SE_MCTS_OK 0             /* the chosen action */
#define SE_MCTS_CUT 1            /* some rollout stopped at max_attempts (the reference keeps
                                    retrying); the search went on with its partial return */
#define SE_MCTS_RAISED 2         /* choose_action raises: argmax over no children at a fully
                                    expanded node without possible actions, or sample_action
                                    raising in _rollout or in the root fallback; the search
                                    ends there; type = SE_SAMPLE_RAISES */
#define SE_MCTS_NEVER_RETURNS 3  /* that sample_action never returns; type = SE_SAMPLE_NO_OTHER_PORT */
typedef struct se_mcts_node {
    int32_t parent;       /* index of the parent node, -1 at the root */
    int32_t type, a, b;   /* the action that led here (0, 0, 0 at the root) */
    int32_t visits;
    int32_t reserved;     /* 0 */
    double total_reward;
} se_mcts_node;
typedef struct se_mcts se_mcts;
/* max_simulations in 1..256; the handle owns the tree scratch ((max_simulations + 1) * n nodes
 * of 24 bytes). Destroy it before its env. */
int se_mcts_create(se_mcts** out, se_env* env, int32_t max_simulations);
int se_mcts_choose(se_mcts* m, int32_t simulations, double c_param, int32_t max_rollout_steps,
                   int32_t max_attempts, int64_t mcts_base, int32_t* type, int32_t* a, int32_t* b,
                   int32_t* status, se_mcts_node* tree, int32_t* tree_count, void* stream);
int se_mcts_destroy(se_mcts* m);

/* se_mcts_choose with navigator playouts (an extension: the reference's playout is its random
 * policy): every leaf is valued by playing the navigator of `nav`, with refuel_below and load as
 * in se_nav_actions, on the simulation's private ship. Outputs, tree layout, ids (mcts_base +
 * (env_id_base + i) * simulations + s), the tree-step draws and the root fallback draw are
 * exactly se_mcts_choose's; only the playout differs. Position k = 0 .. max_rollout_steps - 1 of
 * a playout asks the policy for its action: any status but SE_NAV_OK ends the playout with what it
 * has summed; otherwise the action is stepped, a raising step is skipped and not counted (by the
 * policy's construction there is none), a counted step adds its f64 reward in order and one that
 * reports done ends the playout. There is no attempts budget: the positions bound the loop.
 * Draws: the playout draws what se_rollout_nav draws for ids[r] = id, (k, slot 12) words 1-3 and
 * (k, slot 13) for a partial loss or an arrival. No new slot; word 0 of slot 12 is not read.
 * status: SE_MCTS_OK; SE_MCTS_STUCK where some playout ended without an action (sticky, like
 * SE_MCTS_CUT); SE_MCTS_RAISED and SE_MCTS_NEVER_RETURNS only from the empty argmax and from the
 * root fallback (a navigator playout never raises), and they win over SE_MCTS_STUCK; SE_MCTS_CUT
 * does not occur.
 * Misuse (a null m or nav, load < 0, a NaN c_param, a negative max_rollout_steps or mcts_base,
 * simulations outside 1..max_simulations, ids that overflow int64, misaligned or half-given
 * outputs, a nav made on another env than m's) is SE_EINVAL before any launch and whatever the
 * handles' state. A nav whose ports changed is SE_ESTATE ("the ports changed since se_nav_create:
 * call se_nav_rebuild") and launches nothing; n = 0 is a no-op. refuel_below compares as a double
 * does (NaN never refuels). The env's state and counters are only read. One launch, no
 * allocation, no synchronisation: capturable. */
#define SE_MCTS_STUCK 4   /* some playout ended where the navigator had no action; the search
                             went on with that playout's partial return */
int se_mcts_choose_nav(se_mcts* m, se_nav* nav, double refuel_below, int32_t load,
                       int32_t simulations, double c_param, int32_t max_rollout_steps,
                       int64_t mcts_base, int32_t* type, int32_t* a, int32_t* b, int32_t* status,
                       se_mcts_node* tree, int32_t* tree_count, void* stream);

/* Batched tabular SARSA (agents/sarsa.py): one learner with one dense f64 Q-table in device
 * memory, the env's n envs stepping it together. One se_sarsa_step runs the body of train's
 * inner loop (:255-272) for every env: a fresh env first takes choose_action(state) as its
 * pending action; _try_action (:201-220) steps the pending action and, if it raises, repeats
 * sample_action() + step, max_attempts attempts in all (the reference loops forever);
 * next_action = choose_action(next_state) (:135-165); the update (:187-195)
 *   new = q + lr * ((reward + gamma * next_q) - q)
 * in f64, unfused, in that order, with the step's unrounded f64 reward, keyed by (the state
 * before, the pending action as chosen, also where that action raised and a sampled one was
 * stepped), without terminal masking; then done, ep_len >= max_steps (max_steps > 0; 0: no
 * such cut) or a status other than OK restart the env: a reset (:227-243) with fresh origin
 * and dest, marked fresh. A status other than OK writes nothing to the table. With one port
 * (the reference's reset never returns) the restart leaves the destination None.
 *
 * choose_action: with u = word * 2^-32, u < epsilon (strict) explores with sample_action() on
 * that state; else the first strict maximum of Q, from -inf, over _get_possible_actions
 * (:81-133) in its order: SELECT 0..P-1, the moves (0,-1), (0,1), (-1,0), (1,0), and at a port
 * (the first index whose position matches) TAKE_CARGO 1..min(20, stock), TAKE_FUEL 1..min(20,
 * stock). An untouched table answers SELECT 0. Where nothing compares greater (NaN, -inf) it
 * is sample_action(), as in the reference.
 *
 * Table layout. discretize_state (utils/preprocessing.py:65-90) reads the fuel for both of its
 * buckets ("cargo" in the state dict is the fuel, environment.py:206): cargo_bucket =
 * min(int(fuel / 10), 4), fuel_bucket = min(int(fuel / 20), 4), f64 divisions truncated toward
 * zero. For fuel > -10 seven pairs occur, the fuel class: 0 (0,0), 1 (1,0), 2 (2,1), 3 (3,1),
 * 4 (4,2), 5 (4,3), 6 (4,4). Fuel <= -10 is outside the domain (a move burns at most 1.1 from
 * a non-negative fuel) and is clamped to class 0, as are coordinates and port indices out of
 * range to the nearest valid value / None, so that the index is always in range.
 *   row   = (((x * W + y) * 7 + class) * (P + 1) + origin + 1) * (P + 1) + dest + 1   (None -> 0)
 *   entry = row * A + slot,   A = P + 4 + cmax + 20,   cmax = max(20, the largest port_cargo)
 *   slot: SELECT p at p; the four moves at P..P+3 in the order above; TAKE_CARGO m at P+3+m;
 *         TAKE_FUEL m at P+3+cmax+m.
 * The table (rows * A doubles) is the caller's and zero-initialised by it: the reference's
 * dict answers 0.0 for a key it lacks.
 *
 * Many envs, one table: every Q read of a vector step sees the table after all writes of the
 * step before, and where several envs update one entry in a step the lowest env index
 * (local, i) wins and the others' updates are dropped. With n = 1 or without collisions this
 * is the reference. The handle owns one 4-byte claim word per entry for this.
 *
 * Draws: key (seed, env_id_base + i), the t word the caller's vector-step number t.
 *   slot 20: word 0 the explore uniform of next_action, word 1 its sample_action word,
 *            word 2 the explore uniform of a fresh env's first choice, word 3 its sample word;
 *   slot 21: words 0, 1 the restart's origin and dest, read as se_reset reads its two words;
 *   attempt j of _try_action (j = 0 the pending action): slot 32 + 2j word 0 the
 *   sample_action word (j >= 1), words 1-3 u_fuel, u_gate, u_type; slot 33 + 2j three beta
 *   uniforms and the new destination (a partial loss or an arrival), as se_rollout reads its
 *   two blocks. */
#define SE_SARSA_OK 0             /* a step counted; the table was updated (learn != 0) */
#define SE_SARSA_CUT 1            /* max_attempts attempts raised (the reference keeps trying) */
#define SE_SARSA_RAISED 2         /* a sample_action raised: the reference's train dies there */
#define SE_SARSA_NEVER_RETURNS 3  /* a sample_action never returns (no other port) */
typedef struct se_sarsa_state {   /* caller-owned device SoA, n entries each */
    int32_t* type;                /* the pending action (se_step_typed's encoding) */
    int32_t* a;
    int32_t* b;
    uint8_t* fresh;               /* 1: choose the pending action first (set it after a reset) */
    int32_t* ep_len;              /* counted steps of the running episode */
    double* ep_return;            /* their rewards summed in f64 in order */
} se_sarsa_state;
typedef struct se_sarsa se_sarsa;
/* Fixes the layout for the env's world. P = 0 is refused; SE_EINVAL with the needed byte count
 * in se_last_error() when the table and the claim words (12 bytes per entry) exceed
 * max_table_bytes. After se_set_ports every call but _layout and _destroy returns SE_ESTATE.
 * Destroy the handle before its env. */
int se_sarsa_create(se_sarsa** out, se_env* env, int64_t max_table_bytes);
int se_sarsa_layout(const se_sarsa* s, int64_t* rows, int32_t* A, int32_t* cmax);
/* q: rows * A doubles on the env's device. The struct is copied; the buffers stay the caller's. */
int se_sarsa_bind(se_sarsa* s, double* q, const se_sarsa_state* st);
/* One vector step, asynchronous on the stream. learn = 0 writes no table entry (with
 * epsilon = 0: test_policy's greedy evaluation). Outputs (device, n entries): reward, the
 * counted step's f64 reward (0 where status != OK); ended, 1 where the episode restarted;
 * status, SE_SARSA_*; fin_return / fin_len, the finished episode's return and length where
 * ended. max_attempts in 1..64. The env's step counter advances by one. n = 0: a no-op. Beside
 * the table, the se_sarsa_state fields and the outputs (n entries each) it writes the env's
 * bound state as a step and a reset of the restarted envs do; the done lists are not touched. */
int se_sarsa_step(se_sarsa* s, double lr, double gamma, double epsilon, int32_t learn, int32_t max_steps,
                  int32_t max_attempts, uint32_t t, double* reward, uint8_t* ended, int32_t* status,
                  double* fin_return, int32_t* fin_len, void* stream);
/* choose_action alone from every env's current state, with slot 20's words 2 and 3; type < 0
 * (SE_SAMPLE_*) where its sample_action raises. Nothing is modified. */
int se_sarsa_choose(se_sarsa* s, double epsilon, uint32_t t, int32_t* type, int32_t* a, int32_t* b,
                    void* stream);
int se_sarsa_destroy(se_sarsa* s);

/* The sparse table: a second kind of handle behind the same se_sarsa_step / se_sarsa_choose, for
 * worlds whose dense table does not fit (rows grows with (P + 1)^2). It holds a page of A doubles
 * for every row some update has met and nothing for the others; since the dense table starts as
 * zeros, an absent row IS a row of zeros, and a sparse learner computes what the dense one does,
 * bit for bit: every output, the env state, the learner state, and the table as a map.
 *
 * Layout (caller-owned device memory, like the dense q):
 *   keys:  int64_t[capacity]; -1 is an empty slot, any other value the dense layout's row number.
 *   pages: double[capacity * A]; pages[s * A + slot] is entry (keys[s], slot) of the dense layout.
 *          Zero-initialised by the caller; the pages of empty slots stay zero.
 *   capacity: a power of two >= 64.
 *   home(row) = mix(row) & (capacity - 1), mix the splitmix64 finaliser on the row as uint64_t:
 *          z ^= z >> 30;  z *= 0xbf58476d1ce4e5b9;
 *          z ^= z >> 27;  z *= 0x94d049bb133111eb;
 *          z ^= z >> 31.
 *   Probing is linear with step 1 and wraps from the last slot to slot 0. Nothing is deleted: a
 *   lookup ends at the row, at the first empty slot (the row is absent), or after capacity slots.
 * A caller may preload a table that holds these rules (every key reachable from its home before
 * an empty slot, no key twice) before se_sarsa_bind_sparse.
 *
 * A step reads the table as the step before left it: a missing row's greedy scan answers
 * SELECT 0, its curr_q and next_q are 0.0. With learn != 0 every update then finds its row's
 * page or takes the first empty slot of the row's probe for it (a 64-bit compare-and-swap of -1
 * with the row), and the lowest local env index wins each entry as in the dense kind. An update
 * whose probe finds all capacity slots taken by other rows is dropped and counted; it neither
 * waits nor writes. Where two new rows race for one slot in a step, which of them takes it is a
 * matter of timing: the placement of rows is not reproducible, the table as a map row -> page
 * is. learn = 0 changes no byte of keys or pages. The handle owns capacity * A claim words, n
 * parked updates and the two counters. */
/* As se_sarsa_create (the same refusals, the same layout from se_sarsa_layout: the virtual rows,
 * A, cmax), for a table of `capacity` rows. SE_EINVAL for a capacity that is not a power of two
 * >= 64 or where capacity * A * 12 overflows int64. Allocates capacity * A * 4 + n * 20 + 16
 * bytes on the env's device (nothing for n = 0). */
int se_sarsa_create_sparse(se_sarsa** out, se_env* env, int64_t capacity);
/* keys: capacity entries, pages: capacity * A doubles on the env's device; the struct is copied;
 * the buffers stay the caller's. Counts the occupied slots of keys into `used` (one launch over
 * keys on the null stream, which it synchronises: whatever wrote keys must have finished);
 * `dropped` is kept. Reads keys, writes no caller memory. se_sarsa_bind on a sparse handle and
 * se_sarsa_bind_sparse on a dense one return SE_EINVAL. */
int se_sarsa_bind_sparse(se_sarsa* s, int64_t* keys, double* pages, const se_sarsa_state* st);
/* capacity, the pages taken (occupied slots) and the updates dropped since create, after
 * everything queued on the stream: it synchronises the stream. Any output may be NULL. Reads no
 * caller memory. */
int se_sarsa_sparse_stats(se_sarsa* s, int64_t* capacity, int64_t* used, int64_t* dropped, void* stream);
/* Moves the table into new buffers of new_capacity slots (a power of two >= 64; smaller than the
 * current one is legal while it holds the `used` rows, else SE_EINVAL), which the caller has set
 * to -1 (new_keys, new_capacity entries) and zero (new_pages, new_capacity * A doubles): one
 * launch over the old slots re-inserts every occupied row and copies its page, then the handle
 * takes new claim words (new_capacity * A * 4 bytes, the old ones are freed) and binds the new
 * buffers. `used` carries over, `dropped` is kept. It synchronises the stream before and after.
 * The old keys and pages are only read, and never touched again by the handle; of the new
 * buffers only the slots and pages of the rows moved are written. */
int se_sarsa_sparse_grow(se_sarsa* s, int64_t* new_keys, double* new_pages, int64_t new_capacity, void* stream);
/* Host only, no device, no handle: home(row) for a table of `capacity` slots; -1 for a negative
 * row or a capacity that is not a power of two >= 64. */
int64_t se_sarsa_sparse_home(int64_t row, int64_t capacity);

/* Table-policy rollouts (an extension: the reference has no rollout of its SARSA policy; what it
 * has is restated exactly: choose_action, _try_action's fallback and test_policy's loop): what
 * env src[r] earns if it plays the bound Q-table, dense or sparse, from where it stands, without
 * playing it. Rollout r copies env src[r] (the env's state and counters are only read) and plays
 * positions k = 0 .. steps - 1 on the private ship s under the key (seed, ids ? ids[r] :
 * rollout_base + r). Each lane carries one flag, fallback, clear at position 0. The position:
 *   1. d = the block (k, slot 12), the block every rollout kind draws at position k: word 0 the
 *      sample_action word, words 1-3 u_fuel, u_gate, u_type.
 *   2. The action. With fallback set it is sample_action(s, d[0]). Else, if epsilon > 0, one
 *      block is drawn at (k, slot 22) and the position explores iff word0 * 2^-32 < epsilon (the
 *      strict test of random.random() < self.epsilon), the explored action being
 *      sample_action(s, d[0]); with epsilon == 0 slot 22 is not drawn at all. Otherwise the
 *      action is greedy, se_sarsa_choose's choice with epsilon = 0 on the row of the private
 *      ship's discretised state: the first strict maximum from -inf in _get_possible_actions'
 *      order, an absent sparse row answering SELECT 0, and where nothing compares greater (NaN,
 *      -inf) sample_action(s, d[0]).
 *   3. A sample_action that raises (a negative SE_SAMPLE_* type) ends the rollout as se_rollout's
 *      does: status SE_PLAN_STUCK, stuck_at = k, sample_type the type; the step's words are unused.
 *   4. Otherwise the action is stepped with d's words 1-3 and, for a partial loss or an arrival,
 *      the block (k, slot 13), as se_rollout_plan steps position k. A raising step leaves the ship
 *      untouched and counts in end.raised (the first one's error and position are kept); a counted
 *      step adds its f64 reward to ret[r] in order and 1 to counted[r]; one that reports done
 *      ends the rollout with SE_PLAN_DONE.
 *   5. fallback is _try_action (agents/sarsa.py:201-220) with the positions as its attempts: a
 *      raising step sets it, a counted step clears it. Without it a greedy choice that raises
 *      would raise at every later position, since nothing it reads has changed.
 *   6. Running out of positions is SE_PLAN_END. steps = 0 writes ret 0, counted 0 and
 *      SE_PLAN_END; a bad src[r] writes SE_PLAN_BAD_SRC with the zeros and -1 se_rollout_plan
 *      writes. stuck_at is -1 and sample_type 0 for a rollout that is not stuck.
 * What follows: with epsilon = 1 (every position samples with word 0 of slot 12) the rollout
 * equals se_rollout of the same rollout_base with max_steps = max_attempts = steps, in ret (bits),
 * counted steps and the end ship, DONE as DONE, MAX_STEPS / ATTEMPTS as END, RAISED as STUCK; for
 * any epsilon it equals se_rollout_plan (typed) under the same ids fed the actions it emitted, in
 * ret (bits), counted, raised, first_err, first_err_at, the end ship and DONE / END (a stuck
 * rollout up to stuck_at); the first action at epsilon = 0 is se_sarsa_choose(epsilon = 0)'s for
 * that env (where nothing compares greater both sample, each with its own word: slot 12's here,
 * slot 20's there); and a sparse and a dense table holding the same map give the same bytes.
 *
 * Buffers (device): src, m entries, and ids, m entries or NULL, are only read; ret, counted and
 * status, m entries each, are written whole; of `out` (NULL: nothing more is wanted) every
 * pointer that is not NULL gets m entries (stuck_at, sample_type and the nine of `end`), and
 * act_type, act_a and act_b, all three or none, get elements 0 .. m - 1 of each of their `steps`
 * rows of stride ld (step-major, element k * ld + r, as se_rollout_plan reads them: the action of
 * position k, and type 0, a 0, b 0 for a position not played, a stuck position and a bad
 * source); the ld - m columns behind a row are neither read nor written. A NULL pointer's output
 * is not computed. The call reads the env's bound state and the table and writes none of it: not a
 * byte of the env's state and counters, of q or of keys and pages, of the se_sarsa_state fields,
 * of the handle's claim words and park buffers; it launches neither the claim nor the commit
 * kernel, and neither the env's nor the learner's step number moves.
 * Misuse (m, steps or rollout_base negative; epsilon NaN or negative; a null src, ret, counted
 * or status with m > 0; some but not all of act_type, act_a, act_b; with them ld < m, an array
 * that is not 16-byte aligned or, for steps > 1, ld not a multiple of 4) is SE_EINVAL before any
 * launch, whatever the handle's state, and writes nothing. Then the handle is held to
 * se_sarsa_step's readiness: not bound, or se_set_ports since create, is SE_ESTATE. m = 0 is a
 * no-op. One launch, no allocation, no synchronisation: capturable. */
typedef struct se_table_out {      /* every pointer may be NULL: not wanted */
    int32_t *stuck_at, *sample_type;            /* m entries */
    int32_t *act_type, *act_a, *act_b;          /* step-major [steps][ld] rows as se_rollout_plan reads them;
                                                   positions not played hold type 0, a 0, b 0 */
    int64_t ld;                                  /* row stride of the act_* arrays, >= m, rows 16-byte aligned */
    se_plan_out end;
} se_table_out;
int se_rollout_sarsa(se_sarsa* s, double epsilon, const int32_t* src, int64_t m, const int64_t* ids,
                     int64_t rollout_base, int32_t steps, double* ret, int32_t* counted, int32_t* status,
                     const se_table_out* out, void* stream);

/* DQN policy step fused on the GPU (agents/dqn.py): DQNNetwork 6+4P -> 128 -> 128 -> A
 * (A = 4+P+250, :21-33) evaluated with bf16 MFMA and f32 accumulation on the
 * observation preprocess_state builds (utils/preprocessing.py:25-62; its constant port
 * block is folded into fc1's bias), fused with choose_action (:177-203): the first
 * maximum of Q over is_valid_action (:125-175), and epsilon-greedy exploration
 * (np.random.rand() <= epsilon, then random.choice over the valid actions). The
 * N x A Q matrix never reaches HBM (unless q_out asks for it). */
typedef struct se_qnet se_qnet;
int se_qnet_create(se_qnet** out, se_env* env);
/* Weights: DEVICE f32 arrays in torch nn.Linear layout (weight [out][in], bias [out]):
 * w1 [128][6+4P], b1 [128], w2 [128][128], b2 [128], w3 [A][128], b3 [A]. Packed on the
 * stream (bf16, MFMA fragment order). Call again after se_set_ports (the port block is
 * folded with the ports of that moment; se_policy refuses a stale packing).
 * Worlds of 1..64 ports: the policy keeps each env's valid SELECT rows as one 64-bit
 * word, so more ports return SE_EINVAL ("the fused policy supports 1..64 ports"); the
 * env itself stays usable (se_qtrain_create has the same limit). */
int se_qnet_set_weights(se_qnet* q, const float* w1, const float* b1, const float* w2,
                        const float* b2, const float* w3, const float* b3, void* stream);
/* actions[i]: the agent-index action (se_step input) for every env, n entries; the env's
 * state is only read. Exploration draws
 * Philox(seed, env) at (t, slot 14): word 0 * 2^-32 <= epsilon explores, and word 1
 * picks the k-th valid action (ascending index) uniformly. q_out (optional, NULL):
 * the Q rows as computed, [n][ldq] f32, ldq >= A.
 * Non-finite values (se_policy, se_policy_f32 and se_rollout_qnet alike): the greedy action is
 * the first maximum among the valid rows whose Q compares greater than -inf, so a NaN row
 * never wins (torch's argmax would return it) and +inf wins over every finite row; an env with
 * no such row (every valid Q NaN or -inf) plays action 0. q_out shows the NaN / inf of the
 * weights as computed. A ship whose fuel is not finite as f32 (inf, NaN) has every Q NaN (the
 * fuel's parts are inf and inf - inf): its q_out row is NaN and it plays action 0 (it still
 * explores over its valid actions). A finite fuel so large that the activations overflow f32
 * gives inf / NaN rows as the arithmetic produces them, and the rule above picks among them.
 * An env's non-finite fuel or Q stays in that env: its neighbours in the tile are computed bit
 * for bit as without it. */
int se_policy(se_qnet* q, int32_t* actions, double epsilon, uint32_t t, float* q_out, int64_t ldq,
              void* stream);
/* Repack from the device weights of the last se_qnet_set_weights (same tensors, new values:
 * after an optimizer step). bump (optional, device int32): incremented once on the stream
 * (a training loop's update counter, advanced where the new weights take effect). */
/* choose_action as se_policy, with DQNNetwork evaluated in fp32 as agents/dqn.py:198-200
 * runs it (fp32 weights and activations on v_mfma_f32_32x32x2_f32: exact f32 products,
 * f32 accumulation) instead of bf16: the fp32-faithful mode. Packs its image from the
 * weights of the last se_qnet_set_weights (their current values) on every call. */
int se_policy_f32(se_qnet* q, int32_t* actions, double epsilon, uint32_t t, float* q_out, int64_t ldq,
                  void* stream);
int se_qnet_repack(se_qnet* q, int32_t* bump, void* stream);
int se_qnet_destroy(se_qnet* q);  /* destroy a qnet before the env it was created on */

/* Network-policy rollouts (an extension: the reference values its DQN only by stepping the
 * training envs; what it has is restated exactly: choose_action, and the training loop's break on
 * a raising step): what env src[r] earns if it plays the packed network from where it stands,
 * without playing it. Rollout r copies env src[r] (the env's state and counters are only read)
 * and plays positions k = 0 .. steps - 1 on the private ship s under the key (seed, ids ? ids[r] :
 * rollout_base + r). The position:
 *   1. d = the block (k, slot 12), the block every rollout kind draws at position k. Word 0, the
 *      random policy's sample word, is not read; words 1-3 are u_fuel, u_gate, u_type.
 *   2. The action is choose_action (agents/dqn.py:177-203) on s, exactly as se_policy does it for
 *      an env in that state: the observation row's 6 live inputs (x, y, fuel as f64 -> f32 -> bf16
 *      hi + lo, "cargo" = fuel, origin, dest; the port block folded into fc1's bias), and the
 *      first maximum of Q over is_valid_action. If epsilon > 0, one block is drawn at (k, slot 22)
 *      and the position explores iff word0 * 2^-32 <= epsilon (se_policy's non-strict test, not the
 *      table rollout's strict one), word 1 then picking the j-th valid action, ascending, with
 *      uniform_int(word1, 4 + nsel + cst + fst); with epsilon == 0 slot 22 is not drawn at all.
 *      Word 0 of slot 22 is the table rollout's explore uniform, so equal ids explore at the same
 *      positions in both (up to the one word value that separates < from <=).
 *   3. The agent index is stepped as se_rollout_plan steps position k of an agent-index plan: d's
 *      words 1-3 and, for a partial loss or an arrival, the block (k, slot 13).
 *   4. A counted step adds its f64 reward to ret[r] in order and 1 to counted[r]; one that reports
 *      done ends the rollout with SE_PLAN_DONE.
 *   5. A raising step ends the rollout, as the reference's loop breaks on one (agents/dqn.py:
 *      309-313; its `continue` case, "Destination port must be different", is masked out by
 *      is_valid_action, so no chosen action reaches it): the ship is left untouched, the raise
 *      counts 1 in end.raised with first_err and first_err_at = k, and the status is
 *      SE_PLAN_RAISED. This is what se_replay_end's cut does to a training episode. Under the mask
 *      the reachable raises are a move with no destination and a move off the map.
 *   6. Running out of positions is SE_PLAN_END. steps = 0 writes ret 0, counted 0 and
 *      SE_PLAN_END; a bad src[r] writes SE_PLAN_BAD_SRC with the zeros and -1 se_rollout_plan
 *      writes.
 * What follows. The plan equality: for any epsilon the rollout equals se_rollout_plan under the
 * same ids, in its agent-index encoding, fed the actions it emitted with len[r] = counted + raised,
 * in ret (bits), counted, raised, first_err, first_err_at, the end ship and DONE / END (a RAISED
 * rollout reads as END there). The policy equality: the action of position k is se_policy's action
 * for an env holding the rollout's ship before position k (an explored position: se_policy with
 * epsilon 1 picks by its own word what this picks by slot 22's word 1, the same choice law).
 *
 * mode 0 plays the bf16 network as se_policy evaluates it, from the packed image of the last
 * se_qnet_set_weights / se_qnet_repack. mode 1, the fp32-faithful network of se_policy_f32, is not
 * built: SE_EINVAL ("the fp32-faithful rollout is not built").
 *
 * Buffers (device): src, m entries, and ids, m entries or NULL, are only read; ret, counted and
 * status, m entries each, are written whole; of `out` (NULL: nothing more is wanted) every
 * pointer that is not NULL gets m entries (explored and the nine of `end`), and act gets elements
 * 0 .. m - 1 of each of its `steps` rows of stride ld (step-major, element k * ld + r, as
 * se_rollout_plan reads agent indices: the action of position k, and SE_QROLL_PAD for a position
 * not played and a bad source); the ld - m columns behind a row are neither read nor written. The
 * call reads the env's bound state, the world and the packed image and writes none of it: not a
 * byte of the env's state and counters, of the weights, of the images, of the replay ring or of
 * the policy kernels' visiting-order scratch; neither the env's step number nor any counter moves.
 * Misuse (m, steps or rollout_base negative; epsilon NaN or negative; an unknown mode; a null src,
 * ret, counted or status with m > 0; act with ld < m, not 16-byte aligned or, for steps > 1, ld
 * not a multiple of 4) is SE_EINVAL before any launch, whatever the handle's state, and writes
 * nothing. Then the handle is held to se_policy's readiness: no weights set, or se_set_ports
 * since they were, is SE_ESTATE. A network and world image that together exceed the LDS are
 * SE_EINVAL, as for se_policy. m = 0 is a no-op. One launch, no allocation, no synchronisation:
 * capturable. */
#define SE_PLAN_RAISED 6    /* a step raised: the rollout ended there, the ship untouched */
#define SE_QROLL_PAD (-5)   /* an agent index se_step answers with SE_ERR_BAD_INDEX */
typedef struct se_qnet_out {       /* every pointer may be NULL: not wanted */
    int32_t *act;                  /* step-major [steps][ld] agent indices; positions not played hold SE_QROLL_PAD */
    int64_t ld;                    /* >= m, rows 16-byte aligned, a multiple of 4 when steps > 1 */
    int32_t *explored;             /* m entries: positions that took the explore branch */
    se_plan_out end;
} se_qnet_out;
int se_rollout_qnet(se_qnet* q, int32_t mode /* 0: bf16 as se_policy; 1: fp32-faithful as se_policy_f32 */,
                    double epsilon, const int32_t* src, int64_t m, const int64_t* ids, int64_t rollout_base,
                    int32_t steps, double* ret, int32_t* counted, int32_t* status,
                    const se_qnet_out* out, void* stream);

/* DQN experience replay on the device (agents/dqn.py): remember (:117-123) into a ring of
 * `capacity` transitions (deque(maxlen=memory_size)), and update()'s minibatch (:213-224:
 * random.sample, then the preprocess_state rows as f32). A transition is stored compactly
 * (ship bytes, f32 fuel, action, f32 reward, flags) for s and s'; the constant port block
 * of the rows is rebuilt from the world when sampling. capacity in [max(n, 1), 2^31). */
typedef struct se_replay se_replay;
int se_replay_create(se_replay** out, se_env* env, int64_t capacity);
/* Record s and the agent-index actions of every env: call right before se_step. */
int se_replay_begin(se_replay* r, const int32_t* actions, void* stream);
/* Record reward, done and s' after se_step: appends n transitions (FIFO eviction; the ring
 * never holds more than `capacity`, whether or not capacity is a multiple of n or of 4). A
 * step that raised (err != 0) is stored flagged and never sampled: the reference's loop
 * breaks before remember (:304-309). cut (optional, device u8[n]): 1 where the episode must
 * restart, i.e. the step raised or the episode length (step counter - ep_start) >= max_steps (max_steps > 0 needs an auto-reset
 * env, :281); pass it to se_reset. */
int se_replay_end(se_replay* r, uint8_t* cut, int32_t max_steps, void* stream);
/* The training loop's fused forms (one launch each instead of two):
 * se_policy_record = se_policy (q_out NULL) + se_replay_begin with the chosen actions
 * (remember's state and action, agents/dqn.py:117-123 and :285-291);
 * se_replay_end_reset = se_replay_end + se_reset(cut): the cut episodes restart in the
 * same pass, with the draws se_reset would make (the env's reset epoch advances). */
int se_policy_record(se_qnet* q, se_replay* r, int32_t* actions, double epsilon, uint32_t t, void* stream);
/* se_policy_record with the network in fp32 (se_policy_f32's kernel): the same record. */
int se_policy_record_f32(se_qnet* q, se_replay* r, int32_t* actions, double epsilon, uint32_t t, void* stream);
int se_replay_end_reset(se_replay* r, uint8_t* cut, int32_t max_steps, void* stream);
/* se_step_record = se_step + se_replay_end_reset in one launch: the step kernel writes the
 * ring's reward / done / s' record and restarts the cut envs from the state it holds
 * (env.step + remember + env.reset of the training loop, agents/dqn.py:281-309). Needs an
 * auto-reset env; when n, the ring head / capacity are not multiples of 4 or cut is not
 * 4-byte aligned it makes the two launches instead. Results are identical either way.
 * cut (required here): n bytes, every one written (0 or 1). */
int se_step_record(se_replay* r, const int32_t* actions, uint8_t* cut, int32_t max_steps, void* stream);
int se_replay_size(se_replay* r, int64_t* size, int64_t* capacity);
/* A minibatch of `batch` distinct transitions: batch position j takes logical index
 * perm(j) of a 4-round Feistel permutation of [0, size) keyed by Philox(seed, 2^64 - 1) at
 * (t, slot 15), skipping flagged ones through positions j + B, j + 2B, j + 3B (weight 0 if
 * all four are flagged or beyond size). t is read from t_dev (device u32) when non-NULL, so
 * the launch can be captured in a graph with a device-side update counter. Outputs
 * (device): obs and next_obs [batch][6+4P] f32 rows, actions int64, rewards, dones
 * (1.0 / 0.0) and weights (1.0 / 0.0) f32 [batch]. A weight-0 row is written as zeros
 * throughout: both observation rows (the port block included), the action, the reward and
 * done. size == 0 and batch > size are valid: the rows that find no transition come out at
 * weight 0, and rows past `batch` are not written. Sampling between se_replay_begin (or
 * se_policy_record*) and its se_replay_end* / se_step_record is unsupported: the slots of the
 * pass in flight hold a new s beside an old s' (se_qtrain_step_replay refuses it). */
int se_replay_sample(se_replay* r, int64_t batch, const uint32_t* t_dev, uint32_t t, float* obs,
                     float* next_obs, int64_t* actions, float* rewards, float* dones, float* weights,
                     void* stream);
int se_replay_destroy(se_replay* r);  /* destroy a replay before the env it was created on */

/* The DQN update (agents/dqn.py:206-245) fused on f32 MFMA: two kernels per update.
 * Target y = r + gamma * max_a target(s')[a] * (1 - done), loss = sum w (q - y)^2 / sum w
 * (nn.MSELoss when every w is 1), backward, and one Adam step (torch.optim.Adam, no weight
 * decay) on the online parameters in place. Deterministic: no atomics, fixed summation
 * orders. Parameters: DEVICE f32 tensors of DQNNetwork (hidden 128, torch nn.Linear layout);
 * adam_m / adam_v: zero-initialised tensors of the same shapes (exp_avg, exp_avg_sq).
 * Non-finite values: a row without weight (w = 0, or an action outside [0, A), which counts as
 * w = 0) takes no part whatever it holds: its obs, next_obs, reward and done are not used, so
 * NaN or inf there leaves the loss, the parameters and the moments bit for bit what they are
 * with that row zeroed (se_replay_sample writes such rows as zeros; hand-made minibatches need
 * not). On the rows with weight, non-finite values propagate into the loss and the update as
 * in the reference, with one deliberate difference: max_a over the target's Q rows skips NaN
 * (fmaxf), where torch's max returns it. A NaN target row therefore counts as -inf: y is r +
 * gamma * the largest non-NaN target Q (1 - done), and -inf if every row is NaN. */
typedef struct se_mlp {
    float* w1; float* b1;  /* fc1 [128][6+4P], [128] */
    float* w2; float* b2;  /* fc2 [128][128], [128] */
    float* w3; float* b3;  /* fc3 [A][128], [A]; A = 4+P+250 */
} se_mlp;
typedef struct se_qtrain se_qtrain;
int se_qtrain_create(se_qtrain** out, se_env* env, int64_t max_batch);  /* 1 <= P <= 64 */
/* Bind the parameter sets and build the kernel's images of both networks (fragment order,
 * fc1's port block folded with the env's ports of this moment). */
int se_qtrain_bind(se_qtrain* q, const se_mlp* online, const se_mlp* target, const se_mlp* adam_m,
                   const se_mlp* adam_v, void* stream);
/* Rebuild the images of one network (0 online, 1 target) after its parameters changed
 * outside se_qtrain_step (e.g. the target-network copy, update_target_model :109-111). */
int se_qtrain_pack(se_qtrain* q, int32_t which, void* stream);
/* One update on a minibatch (se_replay_sample's outputs, batch <= max_batch). step_dev:
 * device int32 holding the number of Adam steps already taken (bias correction uses it
 * + 1; the caller increments it). loss_out: device f32. Capturable in a graph. */
int se_qtrain_step(se_qtrain* q, int64_t batch, const float* obs, const float* next_obs, const int64_t* act,
                   const float* rew, const float* done, const float* weight, float gamma, float lr,
                   float beta1, float beta2, float eps, const int32_t* step_dev, float* loss_out,
                   void* stream);
/* se_qtrain_step, then what se_qnet_repack(qn, step_dev) would do, in the same two launches:
 * the first kernel advances step_dev (the second's bias correction then uses it as is),
 * and the second writes the policy's bf16 images (both layouts) from the parameters it
 * has just updated. qn must be packed (se_qnet_set_weights) from the very tensors bound
 * as `online` in se_qtrain_bind, on the same env. Same bits as the two calls. */
int se_qtrain_step_policy(se_qtrain* q, se_qnet* qn, int64_t batch, const float* obs,
                          const float* next_obs, const int64_t* act, const float* rew,
                          const float* done, const float* weight, float gamma, float lr, float beta1,
                          float beta2, float eps, int32_t* step_dev, float* loss_out, void* stream);
/* se_replay_sample then se_qtrain_step_policy (qn nullable: se_qtrain_step) in two launches
 * instead of three: the first kernel draws its own minibatch rows from r's ring, the very
 * transitions se_replay_sample(r, batch, t_dev = ctr) picks, without writing the batch
 * buffers. ctr: device int32[2], both entries = the updates taken so far; the sampler key is
 * ctr[0], the first kernel sets ctr[1] = ctr[0] + 1 (the bias-correction count) and the
 * second copies it back into ctr[0]. t >= 0: the caller's copy of ctr[0] (and the ring's size
 * as recorded on the host), so the first kernel does not wait on those device words; t < 0
 * reads them on the device (a graph capture, whose replays advance ctr). Same bits as the sampler plus the step with
 * step_dev = ctr (then advanced); r must record the same env as q and not be mid-record. */
int se_qtrain_step_replay(se_qtrain* q, se_qnet* qn, se_replay* r, int64_t batch, float gamma, float lr,
                          float beta1, float beta2, float eps, int32_t* ctr, int64_t t, float* loss_out,
                          void* stream);
/* Data-parallel update (one learner per GPU, the same parameters on every rank): se_qtrain_step
 * split at the exchange. se_qtrain_grad writes this rank's gradient sums (before the division
 * by sum w) and {sum w (q - y)^2, sum w} into grad, a device f32 vector of
 * se_qtrain_grad_size(q) floats, and changes no parameter. After an all-reduce(SUM) of grad
 * over the ranks, se_qtrain_apply takes one Adam step from it: the update on the union of
 * the ranks' minibatches (loss = global sum w d^2 / global sum w). Same bias-correction
 * counter as se_qtrain_step (step_dev + 1; the caller increments it). qn (nullable): also
 * write that policy's bf16 images, as se_qtrain_step_policy does. Both capturable. */
int64_t se_qtrain_grad_size(const se_qtrain* q);
int se_qtrain_grad(se_qtrain* q, int64_t batch, const float* obs, const float* next_obs, const int64_t* act,
                   const float* rew, const float* done, const float* weight, float gamma, float* grad,
                   void* stream);
int se_qtrain_apply(se_qtrain* q, se_qnet* qn, const float* grad, float lr, float beta1, float beta2,
                    float eps, const int32_t* step_dev, float* loss_out, void* stream);
int se_qtrain_destroy(se_qtrain* q);  /* destroy before the env it was created on */

/* Episode statistics accumulated by the auto-reset path since the last clear:
 * out[0] = sum of returns, out[1] = episodes, out[2] = sum of lengths (device
 * double[3]). Deterministic: per-wave partials are summed in a fixed order. */
int se_episode_stats(se_env* env, double* out, void* stream);
int se_clear_stats(se_env* env, void* stream);

/* Done lists (auto-reset). Every wave of the step kernel writes the envs it
 * finished, in env order, into its own segment; no global atomics, so the list is
 * deterministic. se_done_layout gives the segment stride and count the done_recs /
 * done_count buffers must be sized for (2 * segments * seg_stride records,
 * 2 * segments counts). se_done_list gives where the most recent step wrote
 * (record offset of its buffer, offset of its counts); that list stays intact
 * while the following step runs (a step writes nothing of the other half, neither
 * records nor counts). Only the first done_count[s] records of segment s
 * are valid: records past the count may be stale, or filler records (env == -1,
 * step == the step counter) that pad a segment's records to whole 128-byte lines
 * (above 2^23 envs, or SHIPENV_DONE_PAD=1 at se_create). se_done_compact copies the
 * valid records contiguously on the stream: exactly *out_count records of out, at most n (an
 * out of n records suffices; the records behind them are not written), and the one int
 * out_count. se_episode_stats writes its three doubles. Neither writes a bound buffer. */
int se_done_layout(se_env* env, int64_t* seg_stride, int32_t* segments);
int se_done_list(se_env* env, int64_t* rec_offset, int64_t* count_offset);
int se_done_compact(se_env* env, se_done_rec* out, int32_t* out_count, void* stream);

/* Step counter / reset epoch (checkpoint-resume; shard replay). */
int se_get_counters(se_env* env, uint64_t* step, uint64_t* epoch);
int se_set_counters(se_env* env, uint64_t step, uint64_t epoch);

int se_destroy(se_env* env);
/* ---- Map loader (host only, no GPU): Environment._initialize_map
 * (shipping/environment.py:45-55) without OpenCV. csrc/mapload.cpp. */

/* The luma (Y) plane of a JPEG as cv2.imread(IMREAD_GRAYSCALE) returns it:
 * baseline / extended / progressive Huffman, 8-bit, 1 or 3 components,
 * libjpeg's accurate integer IDCT. *height / *width are always set on success;
 * `out` (row-major, height*width bytes, may be NULL to query the size) is
 * written when cap is large enough. SE_EINVAL on a corrupt or unsupported file. */
int se_map_decode_luma(const uint8_t* data, size_t len, uint8_t* out, size_t cap,
                       int32_t* height, int32_t* width);
/* gray[row0:row1, col0:col1] -> cv2.resize((W, H), INTER_AREA) (generic,
 * downscaling) -> resized (H*W, may be NULL) and mask = resized > threshold (may be NULL). */
int se_map_area_threshold(const uint8_t* gray, int32_t height, int32_t width, int32_t row0,
                          int32_t row1, int32_t col0, int32_t col1, int32_t H, int32_t W,
                          uint8_t threshold, uint8_t* resized, uint8_t* mask);
/* The whole of _initialize_map: decode, crop rows 50:200 / cols 100:300, INTER_AREA
 * to W x H, > 128. water[x * W + y] = 1 for a non-GROUND cell (x = row, :65). */
int se_map_from_jpeg(const uint8_t* data, size_t len, int32_t H, int32_t W, uint8_t* water);

const char* se_last_error(void);
int se_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
