#pragma once
// plan.h — scripted rollouts (se_rollout_plan): rollout_run with the action read from memory
// instead of sample_action. PlanArgs, plan_load and plan_kernel.
//
// A fragment of shipenv.hip's translation unit, included inside its anonymous
// namespace where this text stood: not a stand-alone header.
// Uses world.h (LdsWorld, stage_world), env_core.h (Ship, Pending, env_key, decode_agent) and
// rollout.h (drawn_step).

// Rollout r plays the plan column r on a private copy of env src[r]: plan position k draws what
// attempt k of se_rollout's rollout with the same id draws (block (k, slot 12) words 1-3, and
// (k, slot 13) for a partial loss or an arrival; word 0, the random policy's, is not read), so
// the plan made of that rollout's attempts reproduces it bit for bit. A raising step leaves the
// ship untouched and is not counted; the counter is the plan position, so nothing shifts.
struct PlanArgs {
    const uint32_t* world;
    WorldDims dims;
    int64_t n, m, ld, rollout_base;
    uint64_t seed;
    int32_t steps;
    se_state st;
    const int32_t* src;
    const int32_t* type;  // typed: the action's type; agent form: the agent index
    const int32_t* a;
    const int32_t* b;
    const int32_t* len;
    const int64_t* ids;
    double* ret;
    int32_t* counted;
    int32_t* status;
    se_plan_out out;  // null pointers: not wanted
};

struct PlanAction {
    int32_t ty, a, b;
};

// The action at element `at` of the plan rows (step-major: a wave reads one contiguous row per
// array), or type 0 where the lane has nothing to read.
template <bool kAgent>
__device__ __forceinline__ PlanAction plan_load(const PlanArgs& A, int64_t at, bool want) {
    PlanAction p{0, 0, 0};
    if (want) {
        p.ty = A.type[at];
        if (!kAgent) {
            p.a = A.a[at];
            p.b = A.b[at];
        }
    }
    return p;
}

// One lane per rollout, the waves in a grid-stride loop with the world staged once per
// workgroup. Step k + 1's actions are in flight while step k runs; the step loop ends when no
// lane of the wave is still playing (one ballot per step).
template <bool kAgent>
__global__ __launch_bounds__(kBlock) void plan_kernel(PlanArgs A) {
    extern __shared__ uint32_t lds[];
    const LdsWorld w = stage_world(A.world, A.dims, lds);
    const int lane = (int)(threadIdx.x & 63u);
    for (int64_t r0 = (int64_t)blockIdx.x * kBlock + (int64_t)(threadIdx.x & ~63u); r0 < A.m;
         r0 += (int64_t)gridDim.x * kBlock) {
        const int64_t r = r0 + lane;
        const bool in = r < A.m;
        const int64_t i = in ? (int64_t)A.src[r] : -1;
        const bool good = in & (i >= 0) & (i < A.n);
        const int64_t ic = good ? i : 0;  // an in-range index for the state loads
        Ship s{-1, -1, 0.0, -1, SE_NONE, SE_NONE};  // what a bad source reports
        int32_t len = 0;
        if (good) {
            s = Ship{A.st.x[ic], A.st.y[ic], A.st.fuel[ic], A.st.cargo[ic], A.st.origin[ic], A.st.dest[ic]};
            len = A.len ? min(max(A.len[r], 0), A.steps) : A.steps;
        }
        const Key key = env_key(A.seed, (good && A.ids) ? A.ids[r] : A.rollout_base + r);
        double total = 0.0;
        int32_t counted = 0, raised = 0, first_err = SE_ERR_OK, first_at = -1;
        int32_t status = good ? SE_PLAN_END : SE_PLAN_BAD_SRC;
        bool alive = len > 0;
        int64_t at = r;  // k * ld + r
        PlanAction cur = plan_load<kAgent>(A, at, alive);
        for (int32_t k = 0; __ballot(alive) != 0ull; ++k) {
            at += A.ld;
            const PlanAction next = plan_load<kAgent>(A, at, alive & (k + 1 < len));
            if (alive) {
                int ty = cur.ty, va = cur.a, vb = cur.b, e_in = SE_ERR_OK;
                if (kAgent) e_in = decode_agent(w.P, cur.ty, ty, va, vb);
                const U4 d = draw(key, (uint32_t)k, kSlotRollout);
                Pending p;
                if (kAgent) {
                    p = drawn_step(w, s, key, (uint32_t)k, kSlotRolloutB, d, ty, va, vb, e_in);
                } else {
                    // a typed move may be of any length: the fuel cost's f64 square root runs only
                    // when some playing lane of the wave moves otherwise than by one cell
                    const bool unit = ((uint32_t)va + 1u <= 2u) & ((uint32_t)vb + 1u <= 2u) & ((va == 0) != (vb == 0));
                    if (__ballot((ty == 1) & !unit) == 0ull)
                        p = drawn_step<false, true>(w, s, key, (uint32_t)k, kSlotRolloutB, d, ty, va, vb);
                    else
                        p = drawn_step<false, false>(w, s, key, (uint32_t)k, kSlotRolloutB, d, ty, va, vb);
                }
                if (p.e != SE_ERR_OK) {
                    first_at = raised == 0 ? k : first_at;
                    first_err = raised == 0 ? p.e : first_err;
                    raised += 1;
                } else {
                    total += p.r;
                    counted += 1;
                    status = p.dead ? SE_PLAN_DONE : status;
                }
                alive = (status != SE_PLAN_DONE) & (k + 1 < len);
            }
            cur = next;
        }
        if (!in) continue;
        A.ret[r] = total;
        A.counted[r] = counted;
        A.status[r] = status;
        if (A.out.raised) A.out.raised[r] = raised;
        if (A.out.first_err) A.out.first_err[r] = first_err;
        if (A.out.first_err_at) A.out.first_err_at[r] = first_at;
        if (A.out.x) A.out.x[r] = s.x;
        if (A.out.y) A.out.y[r] = s.y;
        if (A.out.fuel) A.out.fuel[r] = s.fuel;
        if (A.out.cargo) A.out.cargo[r] = s.cargo;
        if (A.out.origin) A.out.origin[r] = s.origin == SE_NONE ? -1 : s.origin;
        if (A.out.dest) A.out.dest[r] = s.dest == SE_NONE ? -1 : s.dest;
    }
}
