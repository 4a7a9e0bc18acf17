#pragma once
// rollout.h — the reference's random policy and what runs on it: sample_action,
// sample_kernel, drawn_step, rollout_run and rollout_kernel (se_rollout; mcts.h
// steps its trees with the same two functions), and stats_kernel, the episode
// statistics' final sum.
//
// A fragment of shipenv.hip's translation unit, included inside its anonymous
// namespace where this text stood: not a stand-alone header.
// Uses world.h (LdsWorld, stage_world, world_view) and env_core.h (EnvArgs, Ship, load_ship,
// Pending, env_begin / env_finish, env_key, beta_part).

// ------------------------------------------------------------------ random policy
// sample_action() (environment.py:245-263) on one env from one Philox word r.
__device__ __forceinline__ void sample_action(const LdsWorld& w, const Ship& s, uint32_t r, int& type,
                                              int& a, int& b) {
    const int cur = w.port_at(s.x, s.y);  // _get_current_port_idx (:145-153)
    a = 0;
    b = 0;
    if (s.dest == SE_NONE && cur >= 0) {  // :247-253, redraw while == current port
        type = w.P < 2 ? SE_SAMPLE_NO_OTHER_PORT : 2;
        a = pick_other(r, w.P, cur);
    } else if (s.cargo == 0 && cur >= 0) {  // :255-257, randint(1, port_cargo[idx]) :160
        const int stock = w.pcargo(cur);
        type = stock < 1 ? SE_SAMPLE_RAISES : 4;  // randint(1, 0): ValueError
        a = 1 + uniform_int(r, (uint32_t)max(stock, 1));
    } else if (s.fuel == 0.0 && cur >= 0) {  // :258-260: self.fuel[idx] raises TypeError (:163)
        type = SE_SAMPLE_RAISES;
    } else {  // random.choice([NORTH, EAST, SOUTH, WEST]) (:165-167, shipping/type.py:8-16)
        const int k = (int)(r & 3u), odd = k & 1;
        type = 1;
        a = odd * (k - 2);
        b = (1 - odd) * (k - 1);
    }
    if (type < 0) {  // no action: the reference raises / never returns
        a = 0;
        b = 0;
    }
}

struct SampleArgs : EnvArgs {
    uint32_t t;
    int32_t* type;
    int32_t* a;
    int32_t* b;
};

// One cell-code byte and one stock per env: read in place through L1 / L2 instead of
// staging the 10.8 KB image into every one of up to 2048 workgroups.
__global__ __launch_bounds__(kBlock) void sample_kernel(SampleArgs A) {
    const LdsWorld w = world_view(A.dims, A.world);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < A.n;
         i += (int64_t)gridDim.x * kBlock) {
        const Ship s = load_ship(A.st, i);
        const U4 d = draw(env_key(A.seed, A.env_base + i), A.t, kSlotSample);
        int ty, va, vb;
        sample_action(w, s, d.v[0], ty, va, vb);
        A.type[i] = ty;
        A.a[i] = va;
        A.b[i] = vb;
    }
}

// MCTS rollouts (agents/mcts.py:211-238), one per thread: a private copy of env
// src[r], then sample_action + step until done / max_steps counted steps /
// max_attempts attempts. A raising step is retried without counting (:231-233);
// a raising sample_action ends the rollout (it sits outside the try, :227).
struct RolloutArgs : EnvArgs {
    int64_t m, rollout_base;
    int32_t max_steps, max_attempts;
    const int32_t* src;
    double* ret;
    int32_t* steps;
    int32_t* status;
};

// One step of a private env copy from its drawn block d (words 1-3: u_fuel, u_gate, u_type)
// and, for a partial loss or an arrival, the block at (t, slot_b): three beta uniforms, the
// new destination. The step of a rollout attempt and of an MCTS tree step (mcts.h). A
// raising step (p.e != SE_ERR_OK) leaves s untouched. kUnitMoves: the action is one the random
// policy or a decoded agent index can name (a unit move, a port in range, a type in 1..4);
// plan.h's typed plans are not, and its agent plans hand their decode error in as e_in.
template <bool kUnitMoves = true, bool kUnitCost = kUnitMoves>
__device__ __forceinline__ Pending drawn_step(const LdsWorld& w, Ship& s, const Key& key, uint32_t t,
                                              uint32_t slot_b, const U4& d, int ty, int va, int vb,
                                              int e_in = SE_ERR_OK) {
    Pending p = env_begin<kUnitMoves, false, kUnitCost>(w, s, e_in, ty, va, vb, (double)d.v[1], 0.0, d.v[2]);
    if (p.e != SE_ERR_OK) return p;
    const int total_kind = d.v[3] > kTypeHi ? kLossTotal : kLossPartial;
    const int kind = d.v[3] < kTypeLo ? kLossNone : total_kind;
    uint32_t med = 0u;
    int nd = 0;
    if ((p.fires & (kind == kLossPartial)) | p.arrive) {
        const U4 e = draw(key, t, slot_b);
        const uint32_t lo = min(e.v[0], e.v[1]), hi = max(e.v[0], e.v[1]);
        med = max(lo, min(hi, e.v[2]));
        nd = pick_other(e.v[3], w.P, s.dest);
    }
    env_finish(s, p, kind, beta_part(med, s.cargo), nd, p.fires, p.arrive);
    return p;
}

// _rollout (agents/mcts.py:211-238) on the private copy s with the draws of `key`; returns
// SE_ROLL_*. A raising sample_action leaves its type (SE_SAMPLE_*) in sample_type.
__device__ __forceinline__ int32_t rollout_run(const LdsWorld& w, Ship& s, const Key& key, int32_t max_steps,
                                               int32_t max_attempts, double& total, int32_t& steps,
                                               int& sample_type) {
    total = 0.0;
    steps = 0;
    sample_type = 0;
    int32_t status = SE_ROLL_ATTEMPTS;
    for (int32_t k = 0; k < max_attempts; ++k) {
        if (steps >= max_steps) {  // while not done and steps < max_rollout_steps (:225)
            status = SE_ROLL_MAX_STEPS;
            break;
        }
        const U4 d = draw(key, (uint32_t)k, kSlotRollout);
        int ty, va, vb;
        sample_action(w, s, d.v[0], ty, va, vb);
        if (ty < 0) {
            sample_type = ty;
            status = SE_ROLL_RAISED;
            break;
        }
        const Pending p = drawn_step(w, s, key, (uint32_t)k, kSlotRolloutB, d, ty, va, vb);
        if (p.e != SE_ERR_OK) continue;  // except Exception: continue (state untouched)
        total += p.r;  // total_reward += reward (:229)
        steps += 1;
        if (p.dead) {
            status = SE_ROLL_DONE;
            break;
        }
    }
    if (status == SE_ROLL_ATTEMPTS && steps >= max_steps) status = SE_ROLL_MAX_STEPS;
    return status;
}

__global__ __launch_bounds__(kBlock) void rollout_kernel(RolloutArgs A) {
    extern __shared__ uint32_t lds[];
    const LdsWorld w = stage_world(A.world, A.dims, lds);
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < A.m;
         r += (int64_t)gridDim.x * kBlock) {
        const int64_t i = A.src[r];
        if (i < 0 || i >= A.n) {
            A.ret[r] = 0.0;
            A.steps[r] = 0;
            A.status[r] = SE_ROLL_BAD_SRC;
            continue;
        }
        Ship s = load_ship(A.st, i);
        double total;
        int32_t steps;
        int sample_type;
        const int32_t status = rollout_run(w, s, env_key(A.seed, A.rollout_base + r), A.max_steps,
                                           A.max_attempts, total, steps, sample_type);
        A.ret[r] = total;
        A.steps[r] = steps;
        A.status[r] = status;
    }
}

// ------------------------------------------------------------------ stats reduce
// One workgroup sums the per-wave slab entries in a fixed order (thread t takes entries
// t, t + 1024, ... in turn; then a shuffle butterfly per wave and the 16 wave sums in
// wave order), so the result does not depend on timing. The slab has one entry per wave
// of the step grid: 4096 at 2^20 envs, 131072 at 2^25 with one group per thread.
constexpr int kStatsBlock = 1024;
__global__ __launch_bounds__(kStatsBlock) void stats_kernel(const double* __restrict__ slab, int blocks,
                                                            double* __restrict__ out) {
    __shared__ double part[3][kStatsBlock / 64];
    double a = 0.0, b = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < blocks; i += kStatsBlock) {
        a += slab[4 * i];
        b += slab[4 * i + 1];
        c += slab[4 * i + 2];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off);
        b += __shfl_xor(b, off);
        c += __shfl_xor(c, off);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[0][w] = a;
        part[1][w] = b;
        part[2][w] = c;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = 0.0;
        for (int k = 0; k < kStatsBlock / 64; ++k) s += part[threadIdx.x][k];
        out[threadIdx.x] = s;
    }
}
