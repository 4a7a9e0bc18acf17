#pragma once
// plan.h — scripted rollouts (se_rollout_plan): the episode scaffold with the action read from
// memory. PlanArgs, plan_load and plan_kernel.
//
// A fragment of shipenv.hip's translation unit, included inside its anonymous
// namespace where this text stood: not a stand-alone header.
// Uses world.h (LdsWorld, stage_world), env_core.h (Pending, decode_agent), rollout.h
// (drawn_step) and episode.h (EpisodeArgs, episode_lane, EpisodeTally, episode_store).

// Rollout r plays the plan column r on a private copy of env src[r]: plan position k draws what
// attempt k of se_rollout's rollout with the same id draws (block (k, slot 12) words 1-3, and
// (k, slot 13) for a partial loss or an arrival; word 0, the random policy's, is not read), so
// the plan made of that rollout's attempts reproduces it bit for bit. A raising step leaves the
// ship untouched and is not counted; the counter is the plan position, so nothing shifts.
struct PlanArgs : EpisodeArgs {
    int64_t ld;
    int32_t steps;
    const int32_t* type;  // typed: the action's type; agent form: the agent index
    const int32_t* a;
    const int32_t* b;
    const int32_t* len;
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
        EpisodeLane L = episode_lane(A, r0 + lane);
        EpisodeTally T(L);
        int32_t len = 0;
        if (L.good) len = A.len ? min(max(A.len[L.r], 0), A.steps) : A.steps;
        bool alive = len > 0;
        int64_t at = L.r;  // k * ld + r
        PlanAction cur = plan_load<kAgent>(A, at, alive);
        for (int32_t k = 0; __ballot(alive) != 0ull; ++k) {
            at += A.ld;
            const PlanAction next = plan_load<kAgent>(A, at, alive & (k + 1 < len));
            if (alive) {
                int ty = cur.ty, va = cur.a, vb = cur.b, e_in = SE_ERR_OK;
                if (kAgent) e_in = decode_agent(w.P, cur.ty, ty, va, vb);
                const U4 d = draw(L.key, (uint32_t)k, kSlotRollout);
                Pending p;
                if (kAgent) {
                    p = drawn_step(w, L.s, L.key, (uint32_t)k, kSlotRolloutB, d, ty, va, vb, e_in);
                } else {
                    // a typed move may be of any length: the fuel cost's f64 square root runs only
                    // when some playing lane of the wave moves otherwise than by one cell
                    const bool unit = ((uint32_t)va + 1u <= 2u) & ((uint32_t)vb + 1u <= 2u) & ((va == 0) != (vb == 0));
                    if (__ballot((ty == 1) & !unit) == 0ull)
                        p = drawn_step<false, true>(w, L.s, L.key, (uint32_t)k, kSlotRolloutB, d, ty, va, vb);
                    else
                        p = drawn_step<false, false>(w, L.s, L.key, (uint32_t)k, kSlotRolloutB, d, ty, va, vb);
                }
                T.add(p, k);
                alive = !T.done() & (k + 1 < len);
            }
            cur = next;
        }
        if (L.in) episode_store(A, A.out, L, T);
    }
}
