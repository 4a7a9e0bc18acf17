#pragma once
// nav.h — the navigator (an extension: the reference has no such component): the expert policy
// nav_action on the route tables of navfield.h, the two kernels that run it (se_nav_actions on
// the env's state, se_rollout_nav on private copies), and the se_nav handle that builds the
// tables on the host and keeps them on the device; and nav_playout, the rollout's positions for
// one lane, which the MCTS decision kernel plays as its playout.
//
// A fragment of shipenv.hip's translation unit, included at its end before mcts.h (whose
// se_mcts_choose_nav plays nav_playout below): not a stand-alone header.
// Uses world.h (WorldDims, LdsWorld, world_view, stage_world), env_core.h (EnvArgs, Ship,
// load_ship, Pending), rollout.h (drawn_step), episode.h (EpisodeArgs, episode_lane, EpisodeTally,
// episode_store), philox.h, navfield.h, and the host side's se_env, env_args, check_ready, fail,
// HIP_TRY, DeviceGuard, device_reserve, device_free, world_lds, aligned16 (host.h) and grid_for.
//
// The policy and the draw contract are stated in include/shipenv.h. The rollout is episode.h's
// scaffold, as se_rollout_plan is, around nav_position: position k draws what se_rollout_plan's
// position k draws, so a navigated rollout equals the scripted rollout of the actions it emitted.
//
// The dir byte is read from global memory: one dependent byte per step and lane out of a table
// of P * H * W bytes (50 KB at the default world), which stays in L2. Staging the table in LDS
// behind the world image, and issuing the read ahead of the cell-code and stock reads, were both
// measured and not kept: the first is 15 % slower, the second changes nothing.
// No table index is ever formed from a ship outside the map, a dest that names no port or a dir
// byte of SE_NAV_NONE.

namespace {

struct NavTables {
    const uint16_t* field;  // [P][cells]
    const uint8_t* dir;     // [P][cells]
};

struct NavAction {
    int32_t ty, a, b, status;
};

// The navigator's action for ship s (include/shipenv.h has the rules). dist, where wanted, is
// field[dest][cell] or -1.
template <bool kDist = false>
__device__ __forceinline__ NavAction nav_action(const LdsWorld& w, const NavTables& t, const Ship& s,
                                                double refuel_below, int32_t load, int32_t* dist = nullptr) {
    NavAction act{0, 0, 0, SE_NAV_UNREACHABLE};
    if (kDist) *dist = -1;
    if (((unsigned)s.x >= (unsigned)w.H) | ((unsigned)s.y >= (unsigned)w.W)) return act;
    const int32_t cells = mul24i(w.H, w.W);
    const int32_t c = (int32_t)mul24u((uint32_t)s.x, (uint32_t)w.W) + s.y;
    const int cur = w.port_of_code(w.cell[c]);
    if (s.dest == SE_NONE) {
        int best = SE_NAV_INF, pick = -1;
        if (cur >= 0)
            for (int q = 0; q < w.P; ++q) {  // strict less-than in q order: the lowest q wins a tie
                const int f = t.field[(int64_t)q * cells + c];
                if ((q != s.origin) & (f > 0) & (f < best)) {
                    best = f;
                    pick = q;
                }
            }
        if (pick < 0) {
            act.status = SE_NAV_NO_DEST;
            return act;
        }
        return NavAction{2, pick, 0, SE_NAV_OK};
    }
    if ((unsigned)s.dest >= (unsigned)w.P) return act;
    const int64_t at = (int64_t)s.dest * cells + c;
    if (kDist) {
        const int f = t.field[at];
        *dist = f == SE_NAV_INF ? -1 : f;
    }
    if (cur >= 0) {
        const int2 stock = w.stock[cur];
        if ((s.fuel < refuel_below) & (stock.x >= 1)) return NavAction{3, stock.x, 0, SE_NAV_OK};
        if ((s.cargo == 0) & (load > 0) & (stock.y >= 1)) return NavAction{4, min(load, stock.y), 0, SE_NAV_OK};
    }
    const int k = t.dir[at];
    if (k == SE_NAV_NONE) return act;
    const int odd = k & 1;  // decode_agent's moves: N (0,-1), E (-1,0), S (0,1), W (1,0)
    return NavAction{1, odd * (k - 2), (1 - odd) * (k - 1), SE_NAV_OK};
}

// The se_step index of a typed action the navigator emitted, or -1 where there is none: the
// index decodes to TAKE_CARGO 0..49 and TAKE_FUEL 0..199 (decode_agent).
__device__ __forceinline__ int32_t nav_agent_index(int P, const NavAction& act) {
    if (act.status != SE_NAV_OK) return -1;
    if (act.ty == 1) return act.a == 0 ? act.b + 1 : act.a + 2;  // (0,-1) 0, (-1,0) 1, (0,1) 2, (1,0) 3
    if (act.ty == 2) return 4 + act.a;
    if (act.ty == 4) return act.a <= 49 ? 4 + P + act.a : -1;
    return act.a <= 199 ? 54 + P + act.a : -1;
}

// Position k of a navigated rollout on the private ship s under `key`: the navigator's action,
// stepped by drawn_step on the blocks (k, slot 12) and (k, slot 13). On any status but SE_NAV_OK
// the navigator had no action: nothing was drawn or stepped, and p holds nothing. Both the
// rollout kernel and the playout below are made of this. (The step comes back by value: handed
// out through a reference, the rollout kernel's step loop compiled 28 instructions longer.)
struct NavStep {
    int32_t status;  // SE_NAV_*
    Pending p;
};

__device__ __forceinline__ NavStep nav_position(const LdsWorld& w, const NavTables& t, Ship& s, const Key& key,
                                                int32_t k, double refuel_below, int32_t load) {
    const NavAction act = nav_action(w, t, s, refuel_below, load);
    NavStep r;
    r.status = act.status;
    if (act.status == SE_NAV_OK) {
        const U4 d = draw(key, (uint32_t)k, kSlotRollout);
        r.p = drawn_step(w, s, key, (uint32_t)k, kSlotRolloutB, d, act.ty, act.a, act.b);
    }
    return r;
}

// se_rollout_nav's positions for one lane, position for position and draw for draw: the navigator
// played on the private ship s for at most `steps` positions under `key`, the counted steps'
// rewards summed in order into total. A raising step is skipped and not counted (by the policy's
// construction there is none); a counted step that reports done ends it. False where the
// navigator had no action at some position ("stuck"): total is what was summed until then.
// The playout of se_mcts_choose_nav (mcts.h).
__device__ __forceinline__ bool nav_playout(const LdsWorld& w, const NavTables& t, Ship& s, const Key& key,
                                            int32_t steps, double refuel_below, int32_t load, double& total) {
    total = 0.0;
    for (int32_t k = 0; k < steps; ++k) {
        const NavStep st = nav_position(w, t, s, key, k, refuel_below, load);
        if (st.status != SE_NAV_OK) return false;
        const Pending& p = st.p;
        if (p.e != SE_ERR_OK) continue;
        total += p.r;
        if (p.dead) break;
    }
    return true;
}

struct NavActionsArgs : EnvArgs {  // env_base and seed are not read: the policy draws nothing
    NavTables tab;
    double refuel_below;
    int32_t load;
    int32_t *type, *a, *b, *status, *agent, *dist;
};

// One lane per env in a grid-stride loop, the world image read in place as sample_kernel reads
// it: six state fields, one cell-code byte, at most one stock pair and one dir byte per env (a
// ship in port without a destination also reads up to P field values).
__global__ __launch_bounds__(kBlock) void nav_actions_kernel(NavActionsArgs A) {
    const LdsWorld w = world_view(A.dims, A.world);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * kBlock) {
        const Ship s = load_ship(A.st, i);
        int32_t dist;
        const NavAction act = nav_action<true>(w, A.tab, s, A.refuel_below, A.load, &dist);
        A.type[i] = act.ty;
        A.a[i] = act.a;
        A.b[i] = act.b;
        A.status[i] = act.status;
        if (A.agent) A.agent[i] = nav_agent_index(w.P, act);
        if (A.dist) A.dist[i] = dist;
    }
}

struct NavRolloutArgs : EpisodeArgs {
    int32_t steps;
    NavTables tab;
    double refuel_below;
    int32_t load;
    se_nav_out out;  // null pointers: not wanted
};

// One lane per rollout, the waves in a grid-stride loop with the world staged once per
// workgroup; the step loop ends when no lane of the wave is still playing. A position where the
// navigator has no action ends the lane's rollout as stuck.
__global__ __launch_bounds__(kBlock) void nav_rollout_kernel(NavRolloutArgs A) {
    extern __shared__ uint32_t lds[];
    const LdsWorld w = stage_world(A.world, A.dims, lds);
    const int lane = (int)(threadIdx.x & 63u);
    for (int64_t r0 = (int64_t)blockIdx.x * kBlock + (int64_t)(threadIdx.x & ~63u); r0 < A.m;
         r0 += (int64_t)gridDim.x * kBlock) {
        EpisodeLane L = episode_lane(A, r0 + lane);
        EpisodeTally T(L);
        int32_t arrivals = 0, nav_status = SE_NAV_OK, stuck_at = -1;
        bool alive = L.good & (A.steps > 0);
        for (int32_t k = 0; __ballot(alive) != 0ull; ++k) {
            if (alive) {
                const NavStep st = nav_position(w, A.tab, L.s, L.key, k, A.refuel_below, A.load);
                if (st.status != SE_NAV_OK) {
                    T.status = SE_PLAN_STUCK;
                    nav_status = st.status;
                    stuck_at = k;
                    alive = false;
                } else {
                    T.add(st.p, k);
                    arrivals += st.p.arrive ? 1 : 0;  // a raising step has none
                    alive = !T.done() & (k + 1 < A.steps);
                }
            }
        }
        if (!L.in) continue;
        episode_store(A, A.out.end, L, T);
        if (A.out.arrivals) A.out.arrivals[L.r] = arrivals;
        if (A.out.nav_status) A.out.nav_status[L.r] = nav_status;
        if (A.out.stuck_at) A.out.stuck_at[L.r] = stuck_at;
    }
}

}  // namespace

struct se_nav {
    se_env* env = nullptr;  // must outlive the handle (destroy the handle first)
    int device = 0;
    uint64_t world_version = 0;  // of the world the tables were made for; 0: none (a failed rebuild)
    int32_t max_leg = 0;
    std::vector<uint16_t> field;  // the host copy, [P][H * W]
    std::vector<uint8_t> dir;
    uint16_t* d_field = nullptr;
    uint8_t* d_dir = nullptr;
    size_t field_cap = 0, dir_cap = 0;  // bytes allocated
};

namespace {

int nav_ready(const se_nav* h) {
    if (!h) return fail(SE_EINVAL, "null nav handle");
    int rc = check_ready(h->env);
    if (rc) return rc;
    if (h->env->world_version != h->world_version)
        return fail(SE_ESTATE, "the ports changed since se_nav_create: call se_nav_rebuild");
    return SE_OK;
}

// The tables of the env's current world, on the host and then on the device. Until all of it has
// gone through the handle names no world: after a failure every call but a rebuild is SE_ESTATE.
int nav_build(se_nav* h) {
    se_env* env = h->env;
    h->world_version = 0;
    const int32_t P = env->dims.P;
    const size_t count = (size_t)P * (size_t)env->dims.H * (size_t)env->dims.W;
    h->field.assign(count, 0);
    h->dir.assign(count, 0);
    std::string err;
    if (shipenv_nav::build_tables(env->dims.H, env->dims.W, env->water.data(), P, env->port_x.data(),
                                  env->port_y.data(), h->field.data(), h->dir.data(), err))
        return fail(SE_EINVAL, err);
    h->max_leg = shipenv_nav::max_leg(env->dims.H, env->dims.W, P, env->port_x.data(), env->port_y.data(),
                                      h->field.data());
    DeviceGuard g(env->device);
    int rc = device_reserve(h->d_field, h->field_cap, count * sizeof(uint16_t));
    if (rc) return rc;
    rc = device_reserve(h->d_dir, h->dir_cap, count);
    if (rc) return rc;
    if (count > 0) {
        HIP_TRY(hipMemcpy(h->d_field, h->field.data(), count * sizeof(uint16_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->d_dir, h->dir.data(), count, hipMemcpyHostToDevice));
    }
    h->world_version = env->world_version;
    return SE_OK;
}

}  // namespace

extern "C" {

int se_nav_build_host(int32_t H, int32_t W, const uint8_t* water, int32_t P, const int32_t* port_x,
                      const int32_t* port_y, uint16_t* field, uint8_t* dir) {
    std::string err;
    if (shipenv_nav::build_tables(H, W, water, P, port_x, port_y, field, dir, err)) return fail(SE_EINVAL, err);
    return SE_OK;
}

int se_nav_create(se_nav** out, se_env* env) {
    if (!out) return fail(SE_EINVAL, "null out");
    *out = nullptr;
    if (!env) return fail(SE_EINVAL, "null env");
    se_nav* h = new se_nav;
    h->env = env;
    h->device = env->device;
    const int rc = nav_build(h);
    if (rc) {
        const std::string why = g_err;
        se_nav_destroy(h);
        return fail(rc, why);
    }
    *out = h;
    return SE_OK;
}

int se_nav_rebuild(se_nav* h) {
    if (!h) return fail(SE_EINVAL, "null nav handle");
    {
        DeviceGuard g(h->device);
        HIP_TRY(hipDeviceSynchronize());  // the old tables may still be read by queued work
    }
    return nav_build(h);
}

int se_nav_tables(const se_nav* h, const uint16_t** d_field, const uint8_t** d_dir, int32_t* max_leg) {
    if (!h) return fail(SE_EINVAL, "null nav handle");
    if (h->env->world_version != h->world_version)
        return fail(SE_ESTATE, "the ports changed since se_nav_create: call se_nav_rebuild");
    if (d_field) *d_field = h->d_field;
    if (d_dir) *d_dir = h->d_dir;
    if (max_leg) *max_leg = h->max_leg;
    return SE_OK;
}

int se_nav_actions(se_nav* h, double refuel_below, int32_t load, int32_t* type, int32_t* a, int32_t* b,
                   int32_t* status, int32_t* agent, int32_t* dist, void* stream) {
    // the arguments first: misuse is reported whatever the handle's state
    if (load < 0) return fail(SE_EINVAL, "load must be >= 0");
    if (!aligned16(type) || !aligned16(a) || !aligned16(b) || !aligned16(status) || !aligned16(agent) ||
        !aligned16(dist))
        return fail(SE_EINVAL, "navigator arrays must be 16-byte aligned");
    int rc = nav_ready(h);
    if (rc) return rc;
    se_env* env = h->env;
    if (env->n == 0) return SE_OK;
    if (!type || !a || !b || !status) return fail(SE_EINVAL, "null output pointer");
    DeviceGuard g(env->device);
    NavActionsArgs A{};
    static_cast<EnvArgs&>(A) = env_args(env);
    A.tab = NavTables{h->d_field, h->d_dir};
    A.refuel_below = refuel_below;
    A.load = load;
    A.type = type;
    A.a = a;
    A.b = b;
    A.status = status;
    A.agent = agent;
    A.dist = dist;
    nav_actions_kernel<<<grid_for(env->n), kBlock, 0, (hipStream_t)stream>>>(A);
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

int se_rollout_nav(se_nav* h, const int32_t* src, int64_t m, int32_t steps, double refuel_below, int32_t load,
                   const int64_t* ids, int64_t rollout_base, double* ret, int32_t* counted, int32_t* status,
                   const se_nav_out* out, void* stream) {
    // the arguments first: misuse is reported whatever the handle's state
    if (m < 0 || steps < 0 || rollout_base < 0 || load < 0)
        return fail(SE_EINVAL, "m, steps, rollout_base and load must be >= 0");
    if (m > 0 && (!src || !ret || !counted || !status)) return fail(SE_EINVAL, "null rollout buffer");
    if (!aligned16(src) || !aligned16(ids) || !aligned16(ret) || !aligned16(counted) || !aligned16(status))
        return fail(SE_EINVAL, "navigator arrays must be 16-byte aligned");
    if (out) {
        const se_plan_out& e = out->end;
        for (const void* p : {(const void*)out->arrivals, (const void*)out->nav_status, (const void*)out->stuck_at,
                              (const void*)e.raised, (const void*)e.first_err, (const void*)e.first_err_at,
                              (const void*)e.x, (const void*)e.y, (const void*)e.fuel, (const void*)e.cargo,
                              (const void*)e.origin, (const void*)e.dest})
            if (!aligned16(p)) return fail(SE_EINVAL, "navigator arrays must be 16-byte aligned");
    }
    int rc = nav_ready(h);
    if (rc) return rc;
    if (m == 0) return SE_OK;
    se_env* env = h->env;
    DeviceGuard g(env->device);
    size_t lds;
    rc = world_lds<nav_rollout_kernel>(env, lds);
    if (rc) return rc;
    NavRolloutArgs A{};
    static_cast<EpisodeArgs&>(A) = {env_args(env), m, rollout_base, src, ids, ret, counted, status};
    A.steps = steps;
    A.tab = NavTables{h->d_field, h->d_dir};
    A.refuel_below = refuel_below;
    A.load = load;
    if (out) A.out = *out;
    nav_rollout_kernel<<<grid_for(m), kBlock, lds, (hipStream_t)stream>>>(A);
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

int se_nav_destroy(se_nav* h) {
    if (!h) return SE_OK;
    DeviceGuard g(h->device);
    const hipError_t e = device_free({h->d_field, h->d_dir});
    delete h;
    return e == hipSuccess ? SE_OK : fail(SE_EHIP, std::string("hipFree: ") + hipGetErrorString(e));
}

}  // extern "C"
