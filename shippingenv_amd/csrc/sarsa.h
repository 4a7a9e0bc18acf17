#pragma once
// sarsa.h — batched tabular SARSA (agents/sarsa.py): one learner, one dense f64 Q-table in
// HBM, n envs. The table's layout, the discretiser, the greedy scan, the two kernels of a
// vector step, and se_sarsa_create / _layout / _bind / _step / _choose / _destroy.
//
// A fragment of shipenv.hip's translation unit, included at its end after mcts.h: not a
// stand-alone header. Uses world.h (WorldDims, LdsWorld, stage_world), env_core.h (EnvArgs, Ship,
// load_ship / store_ship, Pending, env_key, u32, reset_ship), rollout.h (sample_action,
// drawn_step), philox.h, and the host side's se_env, env_args, check_ready, fail, HIP_TRY,
// DeviceGuard, device_free, world_lds (host.h) and grid_for.
//
// One vector step runs the body of train's inner loop (:255-272) for every env:
//   * a fresh env (after a reset, or restarted by the previous vector step) first takes
//     choose_action(state) as its pending action (:256);
//   * _try_action (:201-220): the pending action is stepped; if it raises, sample_action()
//     and step until one goes through, max_attempts attempts in all (the reference loops
//     forever: running out is SE_SARSA_CUT). A raising sample_action is where the reference's
//     train dies: SE_SARSA_RAISED / SE_SARSA_NEVER_RETURNS;
//   * next_action = choose_action(next_state) (:135-165): with u = word * 2^-32, explore iff
//     u < epsilon (random.random() < self.epsilon, strict), the explored action being
//     sample_action() on the new state; else the first strict maximum of Q over
//     _get_possible_actions (:81-133) in its order: SELECT 0..P-1, the moves (0,-1), (0,1),
//     (-1,0), (1,0), and at a port (the first index whose position matches) TAKE_CARGO
//     1..min(20, stock) then TAKE_FUEL 1..min(20, stock). The scan starts from -inf, so an
//     untouched table answers SELECT 0; where no entry compares greater (all NaN or -inf) the
//     reference falls back to sample_action(), and so does this;
//   * update (:187-195): new = q + lr * ((reward + gamma * next_q) - q) in f64, unfused (the
//     translation unit is built with -ffp-contract=off), with the step's unrounded f64 reward.
//     The key is (state before, the pending action as chosen): when that action raised, the
//     key is still the chosen action, not the substitute that was stepped. No terminal
//     masking: a done step still adds gamma * next_q;
//   * done, ep_len >= max_steps (max_steps > 0; ours: a greedy agent can repeat a legal SELECT
//     forever) or a status other than OK restarts the env: reset (:227-243) with fresh ports,
//     marked fresh. A status other than OK writes nothing to the table. In a world of one port
//     the reference's reset never returns; the restart then leaves the destination None.
//
// discretize_state (utils/preprocessing.py:65-90) as it behaves: state["ship"]["cargo"] is
// the fuel (environment.py:206), so cargo_bucket = min(int(fuel / 10), 4) and fuel_bucket =
// min(int(fuel / 20), 4) both come from the fuel (f64 divisions, truncation toward zero), and
// for fuel > -10 only seven pairs occur: (0,0), (1,0), (2,1), (3,1), (4,2), (4,3), (4,4), the
// fuel class 0..6. A move burns at most 1.1 from a non-negative fuel, so fuel <= -10 does not
// occur; it is clamped to class 0 so that the index is always in range.
//
// Table layout (se_sarsa_layout): row = (((x * W + y) * 7 + class) * (P + 1) + origin + 1) *
// (P + 1) + dest + 1 with None -> 0; entry = row * A + slot, the slot innermost so that one
// state's greedy scan reads contiguous doubles; A = P + 4 + cmax + 20 with cmax = max(20, the
// largest port_cargo) (sample_action takes up to the whole stock). Slots: SELECT p at p, the
// four moves at P..P+3 in the order above, TAKE_CARGO m at P+3+m, TAKE_FUEL m at P+3+cmax+m.
// Zero-initialised by the caller: the reference's dict answers 0.0 for a key it lacks.
//
// Many envs, one table: every Q read of vector step k sees the table after all writes of
// step k-1, and where several envs update one entry in a step the lowest env index wins and
// the others' updates are dropped. Two launches: sarsa_step_kernel reads the table and writes
// none of it, claims owner[entry] with a 32-bit atomicMin of the env index and parks (entry,
// new value); sarsa_commit_kernel writes where the claim is its own and sets the claim word
// back to empty, so the claim table is never cleared. No float atomics, bit-reproducible.
//
// Draw contract: key (seed, env_id_base + i), the t word the caller's vector-step
// number. Slot 20: word 0 the explore uniform of next_action, word 1 its sample_action word,
// word 2 the explore uniform of a fresh env's first choice, word 3 its sample_action word.
// Slot 21: words 0, 1 the restart's origin and dest, as se_reset reads its two words. Attempt
// j of _try_action (j = 0 the pending action): slot 32 + 2j word 0 the sample_action word
// (j >= 1), words 1-3 u_fuel, u_gate, u_type; slot 33 + 2j three beta uniforms and the new
// destination, as drawn_step reads its two blocks.

namespace {

constexpr int kSarsaMaxAttempts = 64;
constexpr uint32_t kSarsaNoOwner = 0xffffffffu;
constexpr int kSarsaClasses = 7;

__device__ __forceinline__ int sarsa_class(double fuel) {
    const int cb = min((int)(fuel / 10.0), 4), fb = min((int)(fuel / 20.0), 4);
    const int c = cb < 4 ? cb : 2 + fb;
    return min(max(c, 0), kSarsaClasses - 1);
}

// the row of a ship's discretised state; a coordinate or port index out of range is clamped
// so that no state, however it was written, indexes outside the table
__device__ __forceinline__ int64_t sarsa_row(const LdsWorld& w, const Ship& s) {
    const int x = min(max(s.x, 0), w.H - 1), y = min(max(s.y, 0), w.W - 1);
    const int o = (unsigned)s.origin < (unsigned)w.P ? s.origin + 1 : 0;
    const int d = (unsigned)s.dest < (unsigned)w.P ? s.dest + 1 : 0;
    const int64_t cell = (int64_t)(x * w.W + y) * kSarsaClasses + sarsa_class(s.fuel);
    return (cell * (w.P + 1) + o) * (w.P + 1) + d;
}

// the slot of a typed action, -1 where the table has none
__device__ __forceinline__ int sarsa_slot(int P, int cmax, int type, int a, int b) {
    if (type == 2) return (unsigned)a < (unsigned)P ? a : -1;
    if (type == 1) {
        if (a == 0 && (b == -1 || b == 1)) return P + (b + 1) / 2;
        if (b == 0 && (a == -1 || a == 1)) return P + 2 + (a + 1) / 2;
        return -1;
    }
    if (type == 4) return (a >= 1 && a <= cmax) ? P + 3 + a : -1;
    if (type == 3) return (a >= 1 && a <= 20) ? P + 3 + cmax + a : -1;
    return -1;
}

__device__ __forceinline__ void sarsa_action(int P, int cmax, int slot, int& type, int& a, int& b) {
    b = 0;
    if (slot < P) {
        type = 2;
        a = slot;
    } else if (slot < P + 4) {  // (0,-1), (0,1), (-1,0), (1,0)
        const int k = slot - P;
        type = 1;
        a = k < 2 ? 0 : 2 * k - 5;
        b = k < 2 ? 2 * k - 1 : 0;
    } else if (slot < P + 4 + cmax) {
        type = 4;
        a = slot - (P + 3);
    } else {
        type = 3;
        a = slot - (P + 3 + cmax);
    }
}

// choose_action (:135-165) on ship s: wu the explore word, ws the sample_action word. A raising
// sample_action leaves its negative SE_SAMPLE_* type.
__device__ __forceinline__ void sarsa_choose(const LdsWorld& w, const double* __restrict__ q, int A, int cmax,
                                             const Ship& s, double epsilon, uint32_t wu, uint32_t ws, int& type,
                                             int& a, int& b) {
    if (u32(wu) < epsilon) {
        sample_action(w, s, ws, type, a, b);
        return;
    }
    const double* row = q + sarsa_row(w, s) * A;
    int best = -1;
    double best_q = -__builtin_inf();
    const int head = w.P + 4;
#pragma unroll 4
    for (int k = 0; k < head; ++k) {
        const double v = row[k];
        if (v > best_q) {
            best_q = v;
            best = k;
        }
    }
    const int cur = w.port_at(s.x, s.y);
    if (cur >= 0) {
        const int nc = min(20, w.pcargo(cur)), nf = min(20, w.pfuel(cur));
        for (int m = 1; m <= nc; ++m) {
            const double v = row[w.P + 3 + m];
            if (v > best_q) {
                best_q = v;
                best = w.P + 3 + m;
            }
        }
        for (int m = 1; m <= nf; ++m) {
            const double v = row[w.P + 3 + cmax + m];
            if (v > best_q) {
                best_q = v;
                best = w.P + 3 + cmax + m;
            }
        }
    }
    if (best < 0) {  // best_action is None (:165)
        sample_action(w, s, ws, type, a, b);
        return;
    }
    sarsa_action(w.P, cmax, best, type, a, b);
}

struct SarsaArgs : EnvArgs {
    uint32_t t;
    se_sarsa_state ag;
    const double* q;
    uint32_t* owner;
    int32_t A, cmax;
    double lr, gamma, epsilon;
    int32_t learn, max_steps, max_attempts;
    int64_t* park_entry;
    double* park_val;
    double* reward;
    uint8_t* ended;
    int32_t* status;
    double* fin_return;
    int32_t* fin_len;
};

__device__ __forceinline__ int32_t sarsa_raise_status(int type) {
    return type == SE_SAMPLE_NO_OTHER_PORT ? SE_SARSA_NEVER_RETURNS : SE_SARSA_RAISED;
}

__global__ __launch_bounds__(kBlock) void sarsa_step_kernel(SarsaArgs A) {
    extern __shared__ uint32_t lds[];
    const LdsWorld w = stage_world(A.world, A.dims, lds);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * kBlock) {
        Ship s = load_ship(A.st, i);
        int ty = A.ag.type[i], va = A.ag.a[i], vb = A.ag.b[i];
        int32_t ep_len = A.ag.ep_len[i];
        double ep_ret = A.ag.ep_return[i];
        const Key key = env_key(A.seed, A.env_base + i);
        const U4 c = draw(key, A.t, kSlotSarsa);
        int32_t status = SE_SARSA_OK;
        // a pending action the table has no slot for was never chosen here: the env is fresh
        if (A.ag.fresh[i] || sarsa_slot(w.P, A.cmax, ty, va, vb) < 0) {
            sarsa_choose(w, A.q, A.A, A.cmax, s, A.epsilon, c.v[2], c.v[3], ty, va, vb);  // :256
            if (ty < 0) status = sarsa_raise_status(ty);
        }
        const int64_t entry = status == SE_SARSA_OK ? sarsa_row(w, s) * A.A + sarsa_slot(w.P, A.cmax, ty, va, vb) : -1;
        // _try_action (:201-220)
        double reward = 0.0;
        bool dead = false, stepped = false;
        if (status == SE_SARSA_OK) {
            int sty = ty, sa = va, sb = vb;
            for (int j = 0; j < A.max_attempts; ++j) {
                const U4 d = draw(key, A.t, kSlotSarsaTry + 2u * (uint32_t)j);
                if (j > 0) {
                    sample_action(w, s, d.v[0], sty, sa, sb);
                    if (sty < 0) {
                        status = sarsa_raise_status(sty);
                        break;
                    }
                }
                const Pending p = drawn_step(w, s, key, A.t, kSlotSarsaTry + 2u * (uint32_t)j + 1u, d, sty, sa, sb);
                if (p.e != SE_ERR_OK) continue;
                reward = p.r;
                dead = p.dead;
                stepped = true;
                break;
            }
            if (!stepped && status == SE_SARSA_OK) status = SE_SARSA_CUT;
        }
        int64_t parked = -1;
        if (status == SE_SARSA_OK) {
            int nty, na, nb;
            sarsa_choose(w, A.q, A.A, A.cmax, s, A.epsilon, c.v[0], c.v[1], nty, na, nb);  // :263
            if (nty < 0) {
                status = sarsa_raise_status(nty);
            } else {
                if (A.learn) {  // update (:187-195)
                    const double curr_q = A.q[entry];
                    const double next_q = A.q[sarsa_row(w, s) * A.A + sarsa_slot(w.P, A.cmax, nty, na, nb)];
                    const double target = reward + A.gamma * next_q;
                    A.park_val[i] = curr_q + A.lr * (target - curr_q);
                    atomicMin(A.owner + entry, (uint32_t)i);
                    parked = entry;
                }
                ty = nty;
                va = na;
                vb = nb;
                ep_ret += reward;
                ep_len += 1;
            }
        }
        if (A.learn) A.park_entry[i] = parked;
        const bool restart = dead || status != SE_SARSA_OK || (A.max_steps > 0 && ep_len >= A.max_steps);
        A.reward[i] = status == SE_SARSA_OK ? reward : 0.0;
        A.ended[i] = (uint8_t)restart;
        A.status[i] = status;
        A.fin_return[i] = restart ? ep_ret : 0.0;
        A.fin_len[i] = restart ? ep_len : 0;
        if (restart) {
            const U4 r = draw(key, A.t, kSlotSarsaReset);
            reset_ship(w, s, r.v[0], r.v[1]);
            if (w.P < 2) s.dest = SE_NONE;
            ep_len = 0;
            ep_ret = 0.0;
        }
        store_ship(A.st, i, s);
        A.ag.type[i] = ty;
        A.ag.a[i] = va;
        A.ag.b[i] = vb;
        A.ag.fresh[i] = (uint8_t)restart;
        A.ag.ep_len[i] = ep_len;
        A.ag.ep_return[i] = ep_ret;
    }
}

// The parked updates whose claim is their own env's; the claim word goes back to empty. A
// loser reads the winner's index or, after the winner's store, empty: never its own.
__global__ __launch_bounds__(kBlock) void sarsa_commit_kernel(int64_t n, const int64_t* __restrict__ park_entry,
                                                              const double* __restrict__ park_val, double* q,
                                                              uint32_t* owner) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t e = park_entry[i];
        if (e < 0) continue;
        if (__hip_atomic_load(owner + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != (uint32_t)i) continue;
        q[e] = park_val[i];
        __hip_atomic_store(owner + e, kSarsaNoOwner, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct SarsaChooseArgs : EnvArgs {
    uint32_t t;
    const double* q;
    int32_t A, cmax;
    double epsilon;
    int32_t* type;
    int32_t* a;
    int32_t* b;
};

__global__ __launch_bounds__(kBlock) void sarsa_choose_kernel(SarsaChooseArgs A) {
    extern __shared__ uint32_t lds[];
    const LdsWorld w = stage_world(A.world, A.dims, lds);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * kBlock) {
        const Ship s = load_ship(A.st, i);
        const U4 c = draw(env_key(A.seed, A.env_base + i), A.t, kSlotSarsa);
        int ty, va, vb;
        sarsa_choose(w, A.q, A.A, A.cmax, s, A.epsilon, c.v[2], c.v[3], ty, va, vb);
        A.type[i] = ty;
        A.a[i] = va;
        A.b[i] = vb;
    }
}

}  // namespace

struct se_sarsa {
    se_env* env = nullptr;  // must outlive the handle (destroy the handle first)
    int device = 0;
    uint64_t world_version = 0;  // of the world the layout was made for
    int64_t n = 0, rows = 0;
    int32_t A = 0, cmax = 0;
    uint32_t* d_owner = nullptr;  // [rows * A] claim words, kSarsaNoOwner between steps
    int64_t* d_park_entry = nullptr;  // [n]
    double* d_park_val = nullptr;     // [n]
    double* q = nullptr;
    se_sarsa_state ag{};
    bool bound = false;
};

namespace {

int sarsa_ready(se_sarsa* h, bool need_bind) {
    if (!h) return fail(SE_EINVAL, "null sarsa handle");
    int rc = check_ready(h->env);
    if (rc) return rc;
    if (h->env->world_version != h->world_version)
        return fail(SE_ESTATE, "the ports changed since se_sarsa_create: the table's layout is stale");
    if (h->env->n != h->n) return fail(SE_EINVAL, "the env's size changed since se_sarsa_create");
    if (need_bind && !h->bound) return fail(SE_ESTATE, "se_sarsa_bind has not been called");
    return SE_OK;
}

}  // namespace

extern "C" {

int se_sarsa_create(se_sarsa** out, se_env* env, int64_t max_table_bytes) {
    if (!out) return fail(SE_EINVAL, "null out");
    *out = nullptr;
    int rc = check_ready(env);
    if (rc) return rc;
    if (env->dims.P < 1) return fail(SE_EINVAL, "SARSA needs at least one port");
    if (env->n >= (int64_t)kSarsaNoOwner) return fail(SE_EINVAL, "SARSA takes fewer than 2^32 - 1 envs");
    if (max_table_bytes < 0) return fail(SE_EINVAL, "max_table_bytes must be >= 0");
    const int P = env->dims.P;
    const int cmax = std::max(20, env->stock_cargo_max);
    const int64_t A = (int64_t)P + 4 + cmax + 20;
    if (A > INT32_MAX) return fail(SE_EINVAL, "a port's cargo stock is too large for a SARSA table");
    // rows * A entries of 8 bytes and a 4-byte claim word each; the products stay far below 2^63
    // (H, W <= 256, P <= 254, stocks < 2^31), but the bytes may exceed what a device holds
    const int64_t rows = (int64_t)env->dims.H * env->dims.W * kSarsaClasses * (P + 1) * (P + 1);
    int64_t entries, bytes;
    if (__builtin_mul_overflow(rows, A, &entries) || __builtin_mul_overflow(entries, (int64_t)12, &bytes))
        return fail(SE_EINVAL, "the SARSA table's size overflows int64");
    if (bytes > max_table_bytes)
        return fail(SE_EINVAL, "the SARSA table and its claim words need " + std::to_string(bytes) +
                                   " bytes, more than max_table_bytes");
    se_sarsa* h = new se_sarsa;
    h->env = env;
    h->device = env->device;
    h->world_version = env->world_version;
    h->n = env->n;
    h->rows = rows;
    h->A = (int32_t)A;
    h->cmax = cmax;
    DeviceGuard g(env->device);
    hipError_t e = hipSuccess;
    if (h->n > 0) {
        e = hipMalloc(&h->d_owner, (size_t)entries * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemset(h->d_owner, 0xff, (size_t)entries * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(&h->d_park_entry, (size_t)h->n * sizeof(int64_t));
        if (e == hipSuccess) e = hipMalloc(&h->d_park_val, (size_t)h->n * sizeof(double));
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        se_sarsa_destroy(h);
        return fail(SE_EHIP, std::string("se_sarsa_create: ") + hipGetErrorString(e));
    }
    *out = h;
    return SE_OK;
}

int se_sarsa_layout(const se_sarsa* h, int64_t* rows, int32_t* A, int32_t* cmax) {
    if (!h) return fail(SE_EINVAL, "null sarsa handle");
    if (rows) *rows = h->rows;
    if (A) *A = h->A;
    if (cmax) *cmax = h->cmax;
    return SE_OK;
}

int se_sarsa_bind(se_sarsa* h, double* q, const se_sarsa_state* st) {
    int rc = sarsa_ready(h, false);
    if (rc) return rc;
    if (!q || !st) return fail(SE_EINVAL, "null argument");
    if (h->n > 0 && (!st->type || !st->a || !st->b || !st->fresh || !st->ep_len || !st->ep_return))
        return fail(SE_EINVAL, "null agent state buffer");
    h->q = q;
    h->ag = *st;
    h->bound = true;
    return SE_OK;
}

int se_sarsa_step(se_sarsa* h, double lr, double gamma, double epsilon, int32_t learn, int32_t max_steps,
                  int32_t max_attempts, uint32_t t, double* reward, uint8_t* ended, int32_t* status,
                  double* fin_return, int32_t* fin_len, void* stream) {
    int rc = sarsa_ready(h, true);
    if (rc) return rc;
    if (!(lr == lr) || !(gamma == gamma) || !(epsilon == epsilon)) return fail(SE_EINVAL, "lr, gamma or epsilon is NaN");
    if (max_steps < 0) return fail(SE_EINVAL, "max_steps must be >= 0");
    if (max_attempts < 1 || max_attempts > kSarsaMaxAttempts) return fail(SE_EINVAL, "max_attempts must be in 1..64");
    se_env* env = h->env;
    if (env->n == 0) return SE_OK;
    if (!reward || !ended || !status || !fin_return || !fin_len) return fail(SE_EINVAL, "null output pointer");
    DeviceGuard g(env->device);
    size_t lds;
    rc = world_lds<sarsa_step_kernel>(env, lds);
    if (rc) return rc;
    SarsaArgs A{};
    static_cast<EnvArgs&>(A) = env_args(env);
    A.t = t;
    A.ag = h->ag;
    A.q = h->q;
    A.owner = h->d_owner;
    A.A = h->A;
    A.cmax = h->cmax;
    A.lr = lr;
    A.gamma = gamma;
    A.epsilon = epsilon;
    A.learn = learn != 0;
    A.max_steps = max_steps;
    A.max_attempts = max_attempts;
    A.park_entry = h->d_park_entry;
    A.park_val = h->d_park_val;
    A.reward = reward;
    A.ended = ended;
    A.status = status;
    A.fin_return = fin_return;
    A.fin_len = fin_len;
    const hipStream_t s = (hipStream_t)stream;
    sarsa_step_kernel<<<grid_for(env->n), kBlock, lds, s>>>(A);
    HIP_TRY(hipGetLastError());
    if (A.learn) {
        sarsa_commit_kernel<<<grid_for(env->n), kBlock, 0, s>>>(env->n, h->d_park_entry, h->d_park_val, h->q, h->d_owner);
        HIP_TRY(hipGetLastError());
    }
    env->step_t += 1;
    return SE_OK;
}

int se_sarsa_choose(se_sarsa* h, double epsilon, uint32_t t, int32_t* type, int32_t* a, int32_t* b, void* stream) {
    int rc = sarsa_ready(h, true);
    if (rc) return rc;
    if (!(epsilon == epsilon)) return fail(SE_EINVAL, "epsilon is NaN");
    se_env* env = h->env;
    if (env->n == 0) return SE_OK;
    if (!type || !a || !b) return fail(SE_EINVAL, "null output pointer");
    DeviceGuard g(env->device);
    size_t lds;
    rc = world_lds<sarsa_choose_kernel>(env, lds);
    if (rc) return rc;
    const SarsaChooseArgs A{env_args(env), t, h->q, h->A, h->cmax, epsilon, type, a, b};
    sarsa_choose_kernel<<<grid_for(env->n), kBlock, lds, (hipStream_t)stream>>>(A);
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

int se_sarsa_destroy(se_sarsa* h) {
    if (!h) return SE_OK;
    DeviceGuard g(h->device);
    const hipError_t e = device_free({h->d_owner, h->d_park_entry, h->d_park_val});
    delete h;
    return e == hipSuccess ? SE_OK : fail(SE_EHIP, std::string("hipFree: ") + hipGetErrorString(e));
}

}  // extern "C"
