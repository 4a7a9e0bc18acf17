#pragma once
// sarsa_rollout.h — table-policy rollouts (an extension: the reference has no rollout of its
// SARSA policy): sarsa_position, one position of a Q-table played on a private ship;
// sarsa_playout, those positions for one lane, shaped like nav_playout; sarsa_rollout_kernel,
// episode.h's scaffold around them for the dense and the sparse table; and se_rollout_sarsa.
//
// A fragment of shipenv.hip's translation unit, included at its end after sarsa.h: not a
// stand-alone header. Uses sarsa.h (SarsaDense, SarsaSparse, SarsaRow, sarsa_row, sarsa_choose,
// se_sarsa, sarsa_ready, sarsa_sparse_table), rollout.h (sample_action through sarsa_choose,
// drawn_step), episode.h (EpisodeArgs, episode_lane, EpisodeTally, episode_store), philox.h and
// the host side's env_args, fail, HIP_TRY, DeviceGuard, world_lds, aligned16 and grid_for.
//
// The position is stated in include/shipenv.h. What it restates of the reference: choose_action
// (agents/sarsa.py:135-165) through sarsa_choose itself, _try_action's fallback (:201-220) with
// the rollout's positions as its attempts, and test_policy's loop (:315-356). Position k draws
// what position k of every rollout kind draws, (k, slot 12) and (k, slot 13), so a table rollout
// equals se_rollout_plan of the actions it emitted and, at epsilon = 1, se_rollout itself. The
// explore uniform alone is new: (k, slot 22) word 0, drawn only where epsilon > 0 and the lane
// is not in its fallback.
//
// Nothing here writes the table, the claim words, the park buffers or the learner state: the
// kernel takes the accessor by value and calls only its find / read.

namespace {

// What position k played: the action (ty < 0: its sample_action raised the SE_SAMPLE_* type,
// nothing was stepped and p holds nothing) and the step.
struct SarsaStep {
    int32_t ty, a, b;
    Pending p;
};

// Position k of a table rollout on the private ship s under `key`. fallback is _try_action's
// state carried between positions: set, the action is sample_action() whatever the table says (a
// raising greedy choice would raise again at every later position: nothing it reads has
// changed); a raising step sets it, a counted step clears it. sarsa_choose does all three
// choices: the fallback is its explore branch taken for certain (epsilon 1 against the uniform
// 0), and with epsilon == 0 the uniform is never below it, so the slot is not drawn.
template <class T>
__device__ __forceinline__ SarsaStep sarsa_position(const LdsWorld& w, const T& table, int A, int cmax, Ship& s,
                                                    const Key& key, int32_t k, double epsilon, bool& fallback) {
    const U4 d = draw(key, (uint32_t)k, kSlotRollout);
    uint32_t wu = 0u;
    if (!fallback && epsilon > 0.0) wu = draw(key, (uint32_t)k, kSlotRolloutQ).v[0];
    SarsaRow<T> row(table, sarsa_row(w, s), A);
    int ty, va, vb;
    sarsa_choose(w, row, cmax, s, fallback ? 1.0 : epsilon, wu, d.v[0], ty, va, vb);
    SarsaStep r;
    r.ty = ty;
    r.a = va;
    r.b = vb;
    if (ty >= 0) {
        r.p = drawn_step(w, s, key, (uint32_t)k, kSlotRolloutB, d, ty, va, vb);
        fallback = r.p.e != SE_ERR_OK;
    }
    return r;
}

// se_rollout_sarsa's positions for one lane, position for position and draw for draw: the table
// played on the private ship s for at most `steps` positions under `key`, the counted steps'
// rewards summed in order into total. A raising step is skipped and not counted; a counted step
// that reports done ends it. False where a sample_action raised at some position ("stuck"): total
// is what was summed until then. Shaped like nav_playout, for a tree search that values its
// leaves with a learned table.
template <class T>
__device__ __forceinline__ bool sarsa_playout(const LdsWorld& w, const T& table, int A, int cmax, Ship& s,
                                              const Key& key, int32_t steps, double epsilon, double& total) {
    total = 0.0;
    bool fallback = false;
    for (int32_t k = 0; k < steps; ++k) {
        const SarsaStep st = sarsa_position(w, table, A, cmax, s, key, k, epsilon, fallback);
        if (st.ty < 0) return false;
        if (st.p.e != SE_ERR_OK) continue;
        total += st.p.r;
        if (st.p.dead) break;
    }
    return true;
}

template <class T>
struct SarsaRolloutArgs : EpisodeArgs {
    int32_t steps;
    T table;
    int32_t A, cmax;
    double epsilon;
    se_table_out out;  // null pointers: not wanted
};

// One lane per rollout, the waves in a grid-stride loop with the world staged once per
// workgroup; the step loop ends when no lane of the wave is still playing. Where the action rows
// are wanted every lane of the wave that names a rollout writes its element of row k, the action
// or zeros, so a row is written once and whole; the rows behind the wave's last position are
// zeros.
template <class T>
__global__ __launch_bounds__(kBlock) void sarsa_rollout_kernel(SarsaRolloutArgs<T> A) {
    extern __shared__ uint32_t lds[];
    const LdsWorld w = stage_world(A.world, A.dims, lds);
    const int lane = (int)(threadIdx.x & 63u);
    const bool acts = A.out.act_type != nullptr;
    for (int64_t r0 = (int64_t)blockIdx.x * kBlock + (int64_t)(threadIdx.x & ~63u); r0 < A.m;
         r0 += (int64_t)gridDim.x * kBlock) {
        EpisodeLane L = episode_lane(A, r0 + lane);
        EpisodeTally T_(L);
        int32_t stuck_at = -1, sample_type = 0;
        bool fallback = false;
        bool alive = L.good & (A.steps > 0);
        int32_t k = 0;
        for (; __ballot(alive) != 0ull; ++k) {
            int32_t ty = 0, va = 0, vb = 0;
            if (alive) {
                const SarsaStep st = sarsa_position(w, A.table, A.A, A.cmax, L.s, L.key, k, A.epsilon, fallback);
                if (st.ty < 0) {
                    T_.status = SE_PLAN_STUCK;
                    sample_type = st.ty;
                    stuck_at = k;
                    alive = false;
                } else {
                    ty = st.ty;
                    va = st.a;
                    vb = st.b;
                    T_.add(st.p, k);
                    alive = !T_.done() & (k + 1 < A.steps);
                }
            }
            if (acts & L.in) {
                const int64_t at = (int64_t)k * A.out.ld + L.r;
                A.out.act_type[at] = ty;
                A.out.act_a[at] = va;
                A.out.act_b[at] = vb;
            }
        }
        if (!L.in) continue;
        if (acts)
            for (; k < A.steps; ++k) {
                const int64_t at = (int64_t)k * A.out.ld + L.r;
                A.out.act_type[at] = 0;
                A.out.act_a[at] = 0;
                A.out.act_b[at] = 0;
            }
        episode_store(A, A.out.end, L, T_);
        if (A.out.stuck_at) A.out.stuck_at[L.r] = stuck_at;
        if (A.out.sample_type) A.out.sample_type[L.r] = sample_type;
    }
}

// the playout is compiled with the library although nothing plays it yet
template __device__ bool sarsa_playout<SarsaDense>(const LdsWorld&, const SarsaDense&, int, int, Ship&, const Key&,
                                                   int32_t, double, double&);
template __device__ bool sarsa_playout<SarsaSparse>(const LdsWorld&, const SarsaSparse&, int, int, Ship&, const Key&,
                                                    int32_t, double, double&);

template <class T>
int sarsa_launch_rollout(se_sarsa* h, const T& table, double epsilon, const EpisodeArgs& E, int32_t steps,
                         const se_table_out* out, hipStream_t s) {
    size_t lds;
    int rc = world_lds<sarsa_rollout_kernel<T>>(h->env, lds);
    if (rc) return rc;
    SarsaRolloutArgs<T> A{};
    static_cast<EpisodeArgs&>(A) = E;
    A.steps = steps;
    A.table = table;
    A.A = h->A;
    A.cmax = h->cmax;
    A.epsilon = epsilon;
    if (out) A.out = *out;
    sarsa_rollout_kernel<T><<<grid_for(E.m), kBlock, lds, s>>>(A);
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

}  // namespace

extern "C" {

int se_rollout_sarsa(se_sarsa* h, double epsilon, const int32_t* src, int64_t m, const int64_t* ids,
                     int64_t rollout_base, int32_t steps, double* ret, int32_t* counted, int32_t* status,
                     const se_table_out* out, void* stream) {
    // the arguments first: misuse is reported whatever the handle's state
    if (m < 0 || steps < 0 || rollout_base < 0) return fail(SE_EINVAL, "m, steps and rollout_base must be >= 0");
    if (!(epsilon >= 0.0)) return fail(SE_EINVAL, "epsilon is NaN or negative");
    if (m > 0 && (!src || !ret || !counted || !status)) return fail(SE_EINVAL, "null rollout buffer");
    if (out) {
        const int wanted = (out->act_type != nullptr) + (out->act_a != nullptr) + (out->act_b != nullptr);
        if (wanted != 0 && wanted != 3) return fail(SE_EINVAL, "act_type, act_a and act_b go together: all or none");
        if (wanted) {
            if (out->ld < m) return fail(SE_EINVAL, "ld must be >= m");
            if (!aligned16(out->act_type) || !aligned16(out->act_a) || !aligned16(out->act_b) ||
                (steps > 1 && (out->ld & 3)))
                return fail(SE_EINVAL, "action rows must be 16-byte aligned (row stride a multiple of 4)");
        }
    }
    int rc = sarsa_ready(h, true);
    if (rc) return rc;
    if (m == 0) return SE_OK;
    se_env* env = h->env;
    DeviceGuard g(env->device);
    const EpisodeArgs E{env_args(env), m, rollout_base, src, ids, ret, counted, status};
    const hipStream_t s = (hipStream_t)stream;
    return h->sparse ? sarsa_launch_rollout(h, sarsa_sparse_table(h), epsilon, E, steps, out, s)
                     : sarsa_launch_rollout(h, SarsaDense{h->q}, epsilon, E, steps, out, s);
}

}  // extern "C"
