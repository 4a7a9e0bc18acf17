#pragma once
// sarsa.h — batched tabular SARSA (agents/sarsa.py): one learner, one f64 Q-table in HBM, n
// envs. The table's layout, the discretiser, the greedy scan, the kernels of a vector step, and
// se_sarsa_create / _layout / _bind / _step / _choose / _destroy. The table is dense (every
// row of the layout) or sparse (se_sarsa_create_sparse / _bind_sparse / _sparse_stats /
// _sparse_grow / _sparse_home: a hash table of the rows met); the step and choose kernels are
// templates over the table accessor, SarsaDense or SarsaSparse.
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
// the others' updates are dropped. The dense kind's two launches: sarsa_step_kernel reads the
// table and writes none of it, claims owner[entry] with a 32-bit atomicMin of the env index and
// parks (entry, new value); sarsa_commit_kernel writes where the claim is its own and sets the
// claim word back to empty, so the claim table is never cleared. No float atomics,
// bit-reproducible.
//
// The sparse table (include/shipenv.h has the contract): keys[capacity] holds -1 or a row
// number, pages[s * A ..] that row's A doubles, the home bucket is the splitmix64 finaliser of the
// row masked to the capacity, probing linear and wrapping, nothing is deleted. An absent row
// reads as zeros: its greedy scan answers SELECT 0 and its curr_q / next_q are 0.0. The step
// kernel looks each of its two states' rows up at most once, reads only, and parks (row, slot,
// new value); with learn != 0 sarsa_claim_kernel then finds or inserts every parked row (a
// 64-bit atomicCAS of -1 -> row, at most `capacity` slots: a full table drops the update, unparks
// it and counts it), rewrites the parked row to the page's entry and claims it with the same
// atomicMin; sarsa_commit_kernel is the dense one on `pages`. Launch boundaries order it all: no
// page is read in the kernel that inserts its key. Which slot a row takes when two new rows race
// for a bucket depends on timing; the table as a map of row -> page does not.
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

// the splitmix64 finaliser: the sparse table's hash of a row number
__host__ __device__ __forceinline__ uint64_t sarsa_mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27;
    z *= 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z;
}

// The table accessors. find(row, A) answers the row's A doubles, null where the table does not
// hold the row (the dense table holds every row); read(page, k) is entry k of a found page.
struct SarsaDense {
    static constexpr bool kSparse = false;
    const double* q;
    __device__ __forceinline__ const double* find(int64_t row, int A) const { return q + row * A; }
    static __device__ __forceinline__ double read(const double* page, int k) { return page[k]; }
};

struct SarsaSparse {
    static constexpr bool kSparse = true;
    const int64_t* keys;
    const double* pages;
    int64_t mask;         // capacity - 1
    int32_t* park_slot;   // [n] the parked update's slot; its row goes to park_entry
    __device__ __forceinline__ const double* find(int64_t row, int A) const {
        int64_t s = (int64_t)(sarsa_mix((uint64_t)row) & (uint64_t)mask);
        for (int64_t k = 0; k <= mask; ++k) {  // a full table without the row ends here
            const int64_t key = keys[s];
            if (key == row) return pages + s * A;
            if (key < 0) return nullptr;
            s = (s + 1) & mask;
        }
        return nullptr;
    }
    static __device__ __forceinline__ double read(const double* page, int k) { return page ? page[k] : 0.0; }
};

// One state's row, looked up at most once (the dense address is arithmetic: nothing to keep).
template <class T>
struct SarsaRow {
    const T& table;
    int64_t row;
    int A;
    const double* page = nullptr;
    bool looked = false;
    __device__ __forceinline__ SarsaRow(const T& t, int64_t r, int a) : table(t), row(r), A(a) {}
    __device__ __forceinline__ const double* get() {
        if constexpr (!T::kSparse) {
            return table.find(row, A);
        } else {
            if (!looked) {
                page = table.find(row, A);
                looked = true;
            }
            return page;
        }
    }
};

// choose_action (:135-165) on ship s, whose row is r: wu the explore word, ws the sample_action
// word. A raising sample_action leaves its negative SE_SAMPLE_* type.
template <class T>
__device__ __forceinline__ void sarsa_choose(const LdsWorld& w, SarsaRow<T>& r, int cmax, const Ship& s,
                                             double epsilon, uint32_t wu, uint32_t ws, int& type, int& a, int& b) {
    if (u32(wu) < epsilon) {
        sample_action(w, s, ws, type, a, b);
        return;
    }
    const double* row = r.get();
    if constexpr (T::kSparse) {
        if (!row) {  // a row of zeros: 0.0 > -inf at SELECT 0, and nothing after it is greater
            sarsa_action(w.P, cmax, 0, type, a, b);
            return;
        }
    }
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

template <class T>
struct SarsaArgs : EnvArgs {
    uint32_t t;
    se_sarsa_state ag;
    T table;
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

template <class T>
__global__ __launch_bounds__(kBlock) void sarsa_step_kernel(SarsaArgs<T> A) {
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
        SarsaRow<T> r0(A.table, sarsa_row(w, s), A.A);  // the state before
        if (A.ag.fresh[i] || sarsa_slot(w.P, A.cmax, ty, va, vb) < 0) {
            sarsa_choose(w, r0, A.cmax, s, A.epsilon, c.v[2], c.v[3], ty, va, vb);  // :256
            if (ty < 0) status = sarsa_raise_status(ty);
        }
        const int slot0 = status == SE_SARSA_OK ? sarsa_slot(w.P, A.cmax, ty, va, vb) : -1;
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
            SarsaRow<T> r1(A.table, sarsa_row(w, s), A.A);  // the state after
            sarsa_choose(w, r1, A.cmax, s, A.epsilon, c.v[0], c.v[1], nty, na, nb);  // :263
            if (nty < 0) {
                status = sarsa_raise_status(nty);
            } else {
                if (A.learn) {  // update (:187-195)
                    const double curr_q = T::read(r0.get(), slot0);
                    const double next_q = T::read(r1.get(), sarsa_slot(w.P, A.cmax, nty, na, nb));
                    const double target = reward + A.gamma * next_q;
                    A.park_val[i] = curr_q + A.lr * (target - curr_q);
                    if constexpr (T::kSparse) {  // sarsa_claim_kernel finds the page and claims
                        A.table.park_slot[i] = slot0;
                        parked = r0.row;
                    } else {
                        const int64_t entry = r0.row * A.A + slot0;
                        atomicMin(A.owner + entry, (uint32_t)i);
                        parked = entry;
                    }
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

// The sparse table's claim: every parked (row, slot) finds its row's page or takes the first
// empty slot of the row's probe for it, then claims the page's entry as the dense step kernel
// claims its own and parks that entry for sarsa_commit_kernel. counters[0] counts the pages
// taken, counters[1] the updates dropped because all `mask + 1` slots held other rows.
__global__ __launch_bounds__(kBlock) void sarsa_claim_kernel(int64_t n, int64_t* keys, int64_t mask, int32_t A,
                                                             int64_t* park_entry, const int32_t* __restrict__ park_slot,
                                                             uint32_t* owner, unsigned long long* counters) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t row = park_entry[i];
        if (row < 0) continue;
        int64_t s = (int64_t)(sarsa_mix((uint64_t)row) & (uint64_t)mask), page = -1;
        for (int64_t k = 0; k <= mask; ++k) {
            int64_t old = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old < 0) {
                old = (int64_t)atomicCAS((unsigned long long*)(keys + s), ~0ull, (unsigned long long)row);
                if (old < 0) {
                    atomicAdd(counters, 1ull);
                    old = row;
                }
            }
            if (old == row) {
                page = s;
                break;
            }
            s = (s + 1) & mask;
        }
        if (page < 0) {  // no room: the update is lost, and counted
            park_entry[i] = -1;
            atomicAdd(counters + 1, 1ull);
            continue;
        }
        const int64_t e = page * A + park_slot[i];
        park_entry[i] = e;
        atomicMin(owner + e, (uint32_t)i);
    }
}

// keys[0 .. capacity) -> counters[0] += the occupied slots (se_sarsa_bind_sparse)
__global__ __launch_bounds__(kBlock) void sarsa_count_kernel(const int64_t* __restrict__ keys, int64_t capacity,
                                                             unsigned long long* counters) {
    unsigned long long mine = 0;
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < capacity; s += (int64_t)gridDim.x * kBlock)
        mine += keys[s] >= 0;
    if (mine) atomicAdd(counters, mine);
}

// se_sarsa_sparse_grow: a block takes kBlock old slots at a time; every occupied one takes the
// first empty slot of its row's probe in the new keys (the rows are distinct, the new table has
// room for all of them: each finds one), then the block copies the pages, A doubles each, with
// consecutive threads on consecutive doubles.
__global__ __launch_bounds__(kBlock) void sarsa_grow_kernel(const int64_t* __restrict__ keys,
                                                            const double* __restrict__ pages, int64_t capacity,
                                                            int64_t* new_keys, double* new_pages, int64_t new_mask,
                                                            int32_t A) {
    __shared__ int64_t to[kBlock];
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < capacity; base += (int64_t)gridDim.x * kBlock) {
        const int64_t s = base + threadIdx.x;
        int64_t dst = -1;
        const int64_t row = s < capacity ? keys[s] : -1;
        if (row >= 0) {
            int64_t d = (int64_t)(sarsa_mix((uint64_t)row) & (uint64_t)new_mask);
            for (int64_t k = 0; k <= new_mask; ++k) {
                if (__hip_atomic_load(new_keys + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0 &&
                    (int64_t)atomicCAS((unsigned long long*)(new_keys + d), ~0ull, (unsigned long long)row) < 0) {
                    dst = d;
                    break;
                }
                d = (d + 1) & new_mask;
            }
        }
        to[threadIdx.x] = dst;
        __syncthreads();
        const int64_t span = (int64_t)kBlock * A;
        for (int64_t j = threadIdx.x; j < span; j += kBlock) {
            const int64_t lane = j / A, k = j - lane * A;
            const int64_t d = to[lane];
            if (d >= 0) new_pages[d * A + k] = pages[(base + lane) * A + k];
        }
        __syncthreads();
    }
}

template <class T>
struct SarsaChooseArgs : EnvArgs {
    uint32_t t;
    T table;
    int32_t A, cmax;
    double epsilon;
    int32_t* type;
    int32_t* a;
    int32_t* b;
};

template <class T>
__global__ __launch_bounds__(kBlock) void sarsa_choose_kernel(SarsaChooseArgs<T> A) {
    extern __shared__ uint32_t lds[];
    const LdsWorld w = stage_world(A.world, A.dims, lds);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * kBlock) {
        const Ship s = load_ship(A.st, i);
        const U4 c = draw(env_key(A.seed, A.env_base + i), A.t, kSlotSarsa);
        int ty, va, vb;
        SarsaRow<T> r(A.table, sarsa_row(w, s), A.A);
        sarsa_choose(w, r, A.cmax, s, A.epsilon, c.v[2], c.v[3], ty, va, vb);
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
    uint32_t* d_owner = nullptr;  // [rows * A] (sparse: [capacity * A]) claim words, kSarsaNoOwner between steps
    int64_t* d_park_entry = nullptr;  // [n]
    double* d_park_val = nullptr;     // [n]
    double* q = nullptr;
    se_sarsa_state ag{};
    bool bound = false;
    // the sparse kind
    bool sparse = false;
    int64_t capacity = 0;
    int64_t* keys = nullptr;   // the caller's, [capacity]
    double* pages = nullptr;   // the caller's, [capacity * A]
    int32_t* d_park_slot = nullptr;            // [n]
    unsigned long long* d_counters = nullptr;  // used, dropped
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

// what both kinds of create refuse, and the layout of the env's world
int sarsa_layout_for(se_sarsa** out, se_env* env, int64_t& rows, int64_t& A, int& cmax) {
    if (!out) return fail(SE_EINVAL, "null out");
    *out = nullptr;
    int rc = check_ready(env);
    if (rc) return rc;
    if (env->dims.P < 1) return fail(SE_EINVAL, "SARSA needs at least one port");
    if (env->n >= (int64_t)kSarsaNoOwner) return fail(SE_EINVAL, "SARSA takes fewer than 2^32 - 1 envs");
    const int P = env->dims.P;
    cmax = std::max(20, env->stock_cargo_max);
    A = (int64_t)P + 4 + cmax + 20;
    if (A > INT32_MAX) return fail(SE_EINVAL, "a port's cargo stock is too large for a SARSA table");
    rows = (int64_t)env->dims.H * env->dims.W * kSarsaClasses * (P + 1) * (P + 1);
    return SE_OK;
}

// the handle with `entries` claim words and the parking places (none of it for n = 0)
int sarsa_new(se_sarsa** out, se_env* env, int64_t rows, int64_t A, int cmax, int64_t entries, int64_t capacity) {
    se_sarsa* h = new se_sarsa;
    h->env = env;
    h->device = env->device;
    h->world_version = env->world_version;
    h->n = env->n;
    h->rows = rows;
    h->A = (int32_t)A;
    h->cmax = cmax;
    h->sparse = capacity > 0;
    h->capacity = capacity;
    DeviceGuard g(env->device);
    hipError_t e = hipSuccess;
    if (h->n > 0) {
        e = hipMalloc(&h->d_owner, (size_t)entries * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemset(h->d_owner, 0xff, (size_t)entries * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(&h->d_park_entry, (size_t)h->n * sizeof(int64_t));
        if (e == hipSuccess) e = hipMalloc(&h->d_park_val, (size_t)h->n * sizeof(double));
        if (h->sparse) {
            if (e == hipSuccess) e = hipMalloc(&h->d_park_slot, (size_t)h->n * sizeof(int32_t));
            if (e == hipSuccess) e = hipMalloc(&h->d_counters, 2 * sizeof(unsigned long long));
            if (e == hipSuccess) e = hipMemset(h->d_counters, 0, 2 * sizeof(unsigned long long));
        }
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        se_sarsa_destroy(h);
        return fail(SE_EHIP, std::string("se_sarsa_create: ") + hipGetErrorString(e));
    }
    *out = h;
    return SE_OK;
}

bool sarsa_capacity_ok(int64_t capacity) { return capacity >= 64 && (capacity & (capacity - 1)) == 0; }

// the two device counters on the host, after everything queued on the stream
int sarsa_counters(se_sarsa* h, hipStream_t s, int64_t& used, int64_t& dropped) {
    unsigned long long c[2] = {0, 0};
    if (h->n > 0) {
        HIP_TRY(hipMemcpyAsync(c, h->d_counters, sizeof(c), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    used = (int64_t)c[0];
    dropped = (int64_t)c[1];
    return SE_OK;
}

template <class T>
int sarsa_launch_step(se_sarsa* h, const T& table, double* values, double lr, double gamma, double epsilon,
                      int32_t learn, int32_t max_steps, int32_t max_attempts, uint32_t t, double* reward,
                      uint8_t* ended, int32_t* status, double* fin_return, int32_t* fin_len, hipStream_t s) {
    se_env* env = h->env;
    size_t lds;
    int rc = world_lds<sarsa_step_kernel<T>>(env, lds);
    if (rc) return rc;
    SarsaArgs<T> A{};
    static_cast<EnvArgs&>(A) = env_args(env);
    A.t = t;
    A.ag = h->ag;
    A.table = table;
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
    sarsa_step_kernel<T><<<grid_for(env->n), kBlock, lds, s>>>(A);
    HIP_TRY(hipGetLastError());
    if (A.learn) {
        if constexpr (T::kSparse) {
            sarsa_claim_kernel<<<grid_for(env->n), kBlock, 0, s>>>(env->n, h->keys, h->capacity - 1, h->A,
                                                                   h->d_park_entry, h->d_park_slot, h->d_owner,
                                                                   h->d_counters);
            HIP_TRY(hipGetLastError());
        }
        sarsa_commit_kernel<<<grid_for(env->n), kBlock, 0, s>>>(env->n, h->d_park_entry, h->d_park_val, values, h->d_owner);
        HIP_TRY(hipGetLastError());
    }
    return SE_OK;
}

template <class T>
int sarsa_launch_choose(se_sarsa* h, const T& table, double epsilon, uint32_t t, int32_t* type, int32_t* a,
                        int32_t* b, hipStream_t s) {
    se_env* env = h->env;
    size_t lds;
    int rc = world_lds<sarsa_choose_kernel<T>>(env, lds);
    if (rc) return rc;
    const SarsaChooseArgs<T> A{env_args(env), t, table, h->A, h->cmax, epsilon, type, a, b};
    sarsa_choose_kernel<T><<<grid_for(env->n), kBlock, lds, s>>>(A);
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

SarsaSparse sarsa_sparse_table(const se_sarsa* h) { return SarsaSparse{h->keys, h->pages, h->capacity - 1, h->d_park_slot}; }

}  // namespace

extern "C" {

int se_sarsa_create(se_sarsa** out, se_env* env, int64_t max_table_bytes) {
    int64_t rows, A;
    int cmax;
    int rc = sarsa_layout_for(out, env, rows, A, cmax);
    if (rc) return rc;
    if (max_table_bytes < 0) return fail(SE_EINVAL, "max_table_bytes must be >= 0");
    // rows * A entries of 8 bytes and a 4-byte claim word each; the products stay far below 2^63
    // (H, W <= 256, P <= 254, stocks < 2^31), but the bytes may exceed what a device holds
    int64_t entries, bytes;
    if (__builtin_mul_overflow(rows, A, &entries) || __builtin_mul_overflow(entries, (int64_t)12, &bytes))
        return fail(SE_EINVAL, "the SARSA table's size overflows int64");
    if (bytes > max_table_bytes)
        return fail(SE_EINVAL, "the SARSA table and its claim words need " + std::to_string(bytes) +
                                   " bytes, more than max_table_bytes");
    return sarsa_new(out, env, rows, A, cmax, entries, 0);
}

int se_sarsa_create_sparse(se_sarsa** out, se_env* env, int64_t capacity) {
    int64_t rows, A;
    int cmax;
    int rc = sarsa_layout_for(out, env, rows, A, cmax);
    if (rc) return rc;
    if (!sarsa_capacity_ok(capacity)) return fail(SE_EINVAL, "a sparse table's capacity must be a power of two >= 64");
    int64_t entries, bytes;
    if (__builtin_mul_overflow(capacity, A, &entries) || __builtin_mul_overflow(entries, (int64_t)12, &bytes))
        return fail(SE_EINVAL, "the SARSA table's size overflows int64");
    return sarsa_new(out, env, rows, A, cmax, entries, capacity);
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
    if (h->sparse) return fail(SE_EINVAL, "se_sarsa_bind on a sparse handle: call se_sarsa_bind_sparse");
    if (!q || !st) return fail(SE_EINVAL, "null argument");
    if (h->n > 0 && (!st->type || !st->a || !st->b || !st->fresh || !st->ep_len || !st->ep_return))
        return fail(SE_EINVAL, "null agent state buffer");
    h->q = q;
    h->ag = *st;
    h->bound = true;
    return SE_OK;
}

int se_sarsa_bind_sparse(se_sarsa* h, int64_t* keys, double* pages, const se_sarsa_state* st) {
    int rc = sarsa_ready(h, false);
    if (rc) return rc;
    if (!h->sparse) return fail(SE_EINVAL, "se_sarsa_bind_sparse on a dense handle: call se_sarsa_bind");
    if (!keys || !pages || !st) return fail(SE_EINVAL, "null argument");
    if (h->n > 0 && (!st->type || !st->a || !st->b || !st->fresh || !st->ep_len || !st->ep_return))
        return fail(SE_EINVAL, "null agent state buffer");
    if (h->n > 0) {  // used = the slots the caller's keys occupy (a preloaded table)
        DeviceGuard g(h->device);
        HIP_TRY(hipMemset(h->d_counters, 0, sizeof(unsigned long long)));
        sarsa_count_kernel<<<grid_for(h->capacity), kBlock, 0, nullptr>>>(keys, h->capacity, h->d_counters);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    h->keys = keys;
    h->pages = pages;
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
    const hipStream_t s = (hipStream_t)stream;
    rc = h->sparse ? sarsa_launch_step(h, sarsa_sparse_table(h), h->pages, lr, gamma, epsilon, learn, max_steps,
                                       max_attempts, t, reward, ended, status, fin_return, fin_len, s)
                   : sarsa_launch_step(h, SarsaDense{h->q}, h->q, lr, gamma, epsilon, learn, max_steps, max_attempts,
                                       t, reward, ended, status, fin_return, fin_len, s);
    if (rc) return rc;
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
    const hipStream_t s = (hipStream_t)stream;
    return h->sparse ? sarsa_launch_choose(h, sarsa_sparse_table(h), epsilon, t, type, a, b, s)
                     : sarsa_launch_choose(h, SarsaDense{h->q}, epsilon, t, type, a, b, s);
}

int se_sarsa_sparse_stats(se_sarsa* h, int64_t* capacity, int64_t* used, int64_t* dropped, void* stream) {
    int rc = sarsa_ready(h, false);
    if (rc) return rc;
    if (!h->sparse) return fail(SE_EINVAL, "se_sarsa_sparse_stats on a dense handle");
    DeviceGuard g(h->device);
    int64_t u, d;
    rc = sarsa_counters(h, (hipStream_t)stream, u, d);
    if (rc) return rc;
    if (capacity) *capacity = h->capacity;
    if (used) *used = u;
    if (dropped) *dropped = d;
    return SE_OK;
}

int se_sarsa_sparse_grow(se_sarsa* h, int64_t* new_keys, double* new_pages, int64_t new_capacity, void* stream) {
    int rc = sarsa_ready(h, true);
    if (rc) return rc;
    if (!h->sparse) return fail(SE_EINVAL, "se_sarsa_sparse_grow on a dense handle");
    if (!new_keys || !new_pages) return fail(SE_EINVAL, "null argument");
    if (!sarsa_capacity_ok(new_capacity)) return fail(SE_EINVAL, "a sparse table's capacity must be a power of two >= 64");
    int64_t entries, bytes;
    if (__builtin_mul_overflow(new_capacity, (int64_t)h->A, &entries) || __builtin_mul_overflow(entries, (int64_t)12, &bytes))
        return fail(SE_EINVAL, "the SARSA table's size overflows int64");
    DeviceGuard g(h->device);
    const hipStream_t s = (hipStream_t)stream;
    int64_t used, dropped;
    rc = sarsa_counters(h, s, used, dropped);  // the steps queued before have run
    if (rc) return rc;
    if (new_capacity < used)
        return fail(SE_EINVAL, "the table holds " + std::to_string(used) + " rows, more than the new capacity");
    if (h->n > 0) {
        uint32_t* owner = nullptr;
        hipError_t e = hipMalloc(&owner, (size_t)entries * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemsetAsync(owner, 0xff, (size_t)entries * sizeof(uint32_t), s);
        if (e == hipSuccess) {
            sarsa_grow_kernel<<<grid_for(h->capacity), kBlock, 0, s>>>(h->keys, h->pages, h->capacity, new_keys,
                                                                       new_pages, new_capacity - 1, h->A);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            (void)device_free({owner});
            return fail(SE_EHIP, std::string("se_sarsa_sparse_grow: ") + hipGetErrorString(e));
        }
        HIP_TRY(device_free({h->d_owner}));
        h->d_owner = owner;
    }
    h->keys = new_keys;
    h->pages = new_pages;
    h->capacity = new_capacity;
    return SE_OK;
}

int64_t se_sarsa_sparse_home(int64_t row, int64_t capacity) {
    if (row < 0 || !sarsa_capacity_ok(capacity)) return -1;
    return (int64_t)(sarsa_mix((uint64_t)row) & (uint64_t)(capacity - 1));
}

int se_sarsa_destroy(se_sarsa* h) {
    if (!h) return SE_OK;
    DeviceGuard g(h->device);
    const hipError_t e = device_free({h->d_owner, h->d_park_entry, h->d_park_val, h->d_park_slot, h->d_counters});
    delete h;
    return e == hipSuccess ? SE_OK : fail(SE_EHIP, std::string("hipFree: ") + hipGetErrorString(e));
}

}  // extern "C"

