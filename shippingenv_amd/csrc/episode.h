#pragma once
// episode.h — what a rollout of numbered positions on a private ship is, whatever chooses its
// actions: EpisodeArgs, the lane (episode_lane), the tally (EpisodeTally) and the store of the
// results (episode_store). plan.h's scripted rollouts, nav.h's navigated rollouts and
// sarsa_rollout.h's table rollouts are this scaffold around their own step loops; a new rollout
// kind plugs in the same way.
//
// A fragment of shipenv.hip's translation unit, included inside its anonymous
// namespace after rollout.h: not a stand-alone header.
// Uses env_core.h (EnvArgs, Ship, load_ship, Pending, env_key).
//
// The contracts that hold through it: rollout r plays on a copy of env src[r] under the key
// (seed, ids ? ids[r] : rollout_base + r) with the position as the counter, so position k of any
// kind draws what position k of every other kind draws (and what attempt k of se_rollout's
// rollout with the same id draws); a raising step is skipped and noted, a counted step adds its
// f64 reward in order, and one that reports done ends the rollout.

// The arguments every kind shares. ids null: rollout r's id is rollout_base + r.
struct EpisodeArgs : EnvArgs {
    int64_t m, rollout_base;
    const int32_t* src;
    const int64_t* ids;
    double* ret;
    int32_t* counted;
    int32_t* status;
};

// One lane's rollout: its index, whether it exists (in) and names an env (good), the private
// ship and the key. A bad source plays nothing and reports the ship below.
struct EpisodeLane {
    int64_t r;
    bool in, good;
    Ship s;
    Key key;
};

__device__ __forceinline__ EpisodeLane episode_lane(const EpisodeArgs& A, int64_t r) {
    EpisodeLane L;
    L.r = r;
    L.in = r < A.m;
    const int64_t i = L.in ? (int64_t)A.src[r] : -1;
    L.good = L.in & (i >= 0) & (i < A.n);
    const int64_t ic = L.good ? i : 0;  // an in-range index for the state loads
    L.s = Ship{-1, -1, 0.0, -1, SE_NONE, SE_NONE};  // what a bad source reports
    if (L.good) L.s = load_ship(A.st, ic);
    L.key = env_key(A.seed, (L.good && A.ids) ? A.ids[r] : A.rollout_base + r);
    return L;
}

// What a rollout has summed and seen so far.
struct EpisodeTally {
    double total = 0.0;
    int32_t counted = 0, raised = 0, first_err = SE_ERR_OK, first_at = -1;
    int32_t status;  // SE_PLAN_END until a counted step reports done; a kind may add its own

    __device__ __forceinline__ explicit EpisodeTally(const EpisodeLane& L)
        : status(L.good ? SE_PLAN_END : SE_PLAN_BAD_SRC) {}

    // The step at position k: a raise is noted (the first one's error and position are kept) and
    // counts nothing; any other step adds its reward in order, and done ends the rollout.
    __device__ __forceinline__ void add(const Pending& p, int32_t k) {
        if (p.e != SE_ERR_OK) {
            first_at = raised == 0 ? k : first_at;
            first_err = raised == 0 ? p.e : first_err;
            raised += 1;
        } else {
            total += p.r;
            counted += 1;
            status = p.dead ? SE_PLAN_DONE : status;
        }
    }

    __device__ __forceinline__ bool done() const { return status == SE_PLAN_DONE; }
};

// ret, counted and status, and what of se_plan_out is wanted (null pointers: not wanted).
__device__ __forceinline__ void episode_store(const EpisodeArgs& A, const se_plan_out& E, const EpisodeLane& L,
                                              const EpisodeTally& T) {
    const int64_t r = L.r;
    const Ship& s = L.s;
    A.ret[r] = T.total;
    A.counted[r] = T.counted;
    A.status[r] = T.status;
    if (E.raised) E.raised[r] = T.raised;
    if (E.first_err) E.first_err[r] = T.first_err;
    if (E.first_err_at) E.first_err_at[r] = T.first_at;
    if (E.x) E.x[r] = s.x;
    if (E.y) E.y[r] = s.y;
    if (E.fuel) E.fuel[r] = s.fuel;
    if (E.cargo) E.cargo[r] = s.cargo;
    if (E.origin) E.origin[r] = s.origin == SE_NONE ? -1 : s.origin;
    if (E.dest) E.dest[r] = s.dest == SE_NONE ? -1 : s.dest;
}
