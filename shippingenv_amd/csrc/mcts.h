#pragma once
// mcts.h — one MCTS decision per env (agents/mcts.py:240-292, MCTSAgent.choose_action):
// the tree in a buffer the handle owns, its kernel, and se_mcts_create / se_mcts_choose /
// se_mcts_destroy.
//
// A fragment of shipenv.hip's translation unit, included at its end after qpolicy.h and nav.h:
// not a stand-alone header. Uses world.h (WorldDims, LdsWorld, stage_world, sqrt_rn), env_core.h
// (EnvArgs, Ship, load_ship, Pending, env_key), rollout.h (sample_action, drawn_step, rollout_run),
// nav.h (NavTables, nav_playout, se_nav, nav_ready), philox.h, and the host side's se_env, env_args,
// check_ready, fail, HIP_TRY, DeviceGuard, aligned16, device_free and world_lds (host.h).
//
// One lane runs choose_action for one env: S = num_simulations sequential simulations
// (selection by UCB1, one expansion, a random rollout, backpropagation) on a private Ship
// copy, then best_child(c_param=0) over the root's children. The env's state is only read.
// A tree step is drawn_step and the rollout is rollout_run, the code of se_rollout: a step
// here is the step everywhere. The kernel is a template over the playout: MctsRandomPlayout is
// the reference's (se_mcts_choose); MctsNavPlayout values a leaf with the navigator instead
// (se_mcts_choose_nav, an extension), nav.h's nav_playout on the same private Ship. Everything
// but the playout is one text for both.
//
// The reference, restated with its quirks:
//   * is_terminal() is never true: _build_state has no "done" key (environment.py:202-225),
//     so selection stops only at a node that is not fully expanded, at a step that reports
//     done (:265) or at a step that raises (:267); expansion then happens from that node with
//     whatever state the env copy has, and a dead ship is stepped further.
//   * get_possible_actions (:50-89) reads the node's stored state, the snapshot taken when the
//     node was expanded (the root's: the env's current state), not the env copy, which replays
//     the path with fresh draws and may be elsewhere. current_port_idx is origin_port_index;
//     state["ship"]["cargo"] is the fuel (environment.py:206). So: dest None -> SELECT of every
//     port but origin, ascending; else fuel == 0 and origin not None -> TAKE_CARGO
//     1..port_cargo[origin] (the TAKE_FUEL branch is unreachable); else the four moves
//     [0,-1], [0,1], [-1,0], [1,0]. A node keeps its parent, its action (as the index into the
//     parent's possible actions), origin, dest, a fuel-was-zero bit, visits and total_reward.
//   * is_fully_expanded compares counts (:48), get_untried_actions compares actions (:102-107):
//     the children's actions are distinct entries of the possible list, so the untried ones are
//     the indices no child holds, and random.choice(untried) is the k-th of them in order.
//   * an expansion step that raises abandons the simulation (continue, :278): no rollout, no
//     backpropagation. A child starts with total_reward = reward (:145).
//   * the rollout starts from the env copy's state (:282); its return is added along the path
//     (:149-159).
//
// Draw contract: simulation s of env i draws from Philox(seed, id),
// id = mcts_base + (env_id_base + i) * S + s. Tree step d of the simulation (selection steps,
// then the expansion step, d from 0) reads block (d, slot 18): word 0 picks among the untried
// actions (the expansion step alone reads it), words 1-3 are u_fuel, u_gate, u_type; and, for
// a partial loss or an arrival, block (d, slot 19): three beta uniforms, the new destination.
// The rollout draws what se_rollout draws for rollout_base + r = id: (attempt, slots 12, 13).
// The root fallback (:292) reads word 0 of (0xFFFFFFFF, slot 18) of simulation 0's key.
// The navigator playout draws what se_rollout_nav draws for ids[r] = id: (position, slot 12)
// words 1-3 and (position, slot 13); word 0 of slot 12 is not read.
//
// Tree storage: SoA [node][env] in a scratch buffer the handle owns, so the lanes of a wave
// touch neighbouring addresses ("MCTS decisions"): a 16-byte record per node and
// env (the node word, the action index, visits) and its f64 total_reward. Children are found
// by scanning the nodes for a parent index.

namespace {

constexpr int kMctsBlock = 64;      // one wave per workgroup: a decision is long and serial
constexpr int kMctsMaxBlocks = 8192;
constexpr int kMctsMaxSims = 256;

// node word: parent (9 bits, kMctsNoParent at the root) | origin << 9 | dest << 17 | fuel-was-zero << 25
constexpr uint32_t kMctsNoParent = 0x1ffu;
__device__ __forceinline__ uint32_t mcts_pack(uint32_t parent, const Ship& s) {
    return parent | ((uint32_t)s.origin & 0xffu) << 9 | ((uint32_t)s.dest & 0xffu) << 17 |
           (s.fuel == 0.0 ? 1u << 25 : 0u);
}

// len(get_possible_actions()) (:50-89) of a node. An origin that names no port makes
// port["cargo"] raise (IndexError): no action, and the empty argmax reports the raise.
__device__ __forceinline__ int mcts_possible(const LdsWorld& w, uint32_t node) {
    const int origin = (int)(node >> 9 & 0xffu), dest = (int)(node >> 17 & 0xffu);
    if (dest == SE_NONE) return w.P - (origin < w.P ? 1 : 0);       // :64-67
    if ((node >> 25 & 1u) && origin != SE_NONE)                     // :70-73
        return origin < w.P ? max(w.pcargo(origin), 0) : 0;
    return 4;                                                       // :80-87
}

// get_possible_actions()[k] of a node as a typed action
__device__ __forceinline__ void mcts_action(const LdsWorld& w, uint32_t node, int k, int& type, int& a, int& b) {
    const int origin = (int)(node >> 9 & 0xffu), dest = (int)(node >> 17 & 0xffu);
    b = 0;
    if (dest == SE_NONE) {
        type = 2;
        a = k + ((origin < w.P && k >= origin) ? 1 : 0);
    } else if ((node >> 25 & 1u) && origin != SE_NONE) {
        type = 4;
        a = k + 1;
    } else {  // [0,-1], [0,1], [-1,0], [1,0]
        type = 1;
        a = k < 2 ? 0 : 2 * k - 5;
        b = k < 2 ? 2 * k - 1 : 0;
    }
}

struct MctsArgs : EnvArgs {
    int64_t mcts_base;
    int32_t sims, max_steps, max_attempts;
    double c;
    const double* logtab;  // [sims + 1]: log(v) from the host's C library, v >= 1
    int4* rec;             // [sims + 1][n]: node word, index into the parent's possible actions, visits, 0
    double* total;         // [sims + 1][n]
    int32_t* type;
    int32_t* a;
    int32_t* b;
    int32_t* status;
    se_mcts_node* tree;
    int32_t* tree_count;
};

// What one pass over the nodes finds of a node's children: how many, best_child(c), and the
// action indices below 64 they hold.
struct MctsKids {
    int nch, best;
    uint64_t tried;
};

// The children of `node` among nodes 1..count-1 in creation order (the order of
// node.children) and best_child(c) (:109-128), the first maximum of UCB1. pv = node.visits.
// A child with visits > 0 was backpropagated through its parent, so parent.visits >=
// child.visits >= 1: parent.visits == 0 cannot reach the formula.
// The nodes are read four at a time, every load of a round issued before the first is used: a
// load per node, each waiting for the one before, made the pass a chain of memory latencies.
constexpr int kMctsScan = 4;
__device__ __forceinline__ MctsKids mcts_children(const MctsArgs& A, int64_t i, int node, int count, double c,
                                                  int pv) {
    const double log_pv = A.logtab[max(pv, 1)];
    MctsKids r{0, 0, 0ull};
    double best_u = 0.0;
    for (int j0 = 1; j0 < count; j0 += kMctsScan) {
        int4 m[kMctsScan];
        double tot[kMctsScan];
#pragma unroll
        for (int k = 0; k < kMctsScan; ++k) {  // past the end: the last node again, not used
            const int64_t at = (int64_t)min(j0 + k, count - 1) * A.n + i;
            m[k] = A.rec[at];
            tot[k] = A.total[at];
        }
#pragma unroll
        for (int k = 0; k < kMctsScan; ++k) {
            if (j0 + k >= count || (int)((uint32_t)m[k].x & kMctsNoParent) != node) continue;
            const int v = m[k].z;
            double u = __builtin_inf();  // visits == 0 (:121-122)
            if (v != 0) {
                const double exploit = tot[k] / (double)v;  // :124-126, f64, in this order
                u = exploit + c * sqrt_rn(2.0 * log_pv / (double)v);
            }
            if (r.nch == 0 || u > best_u) {  // np.argmax: the first maximum
                best_u = u;
                r.best = j0 + k;
            }
            r.tried |= (uint32_t)m[k].y < 64u ? 1ull << (m[k].y & 63) : 0ull;
            ++r.nch;
        }
    }
    return r;
}

// The k-th (from 0) index of 0, 1, ... that no child of `node` holds. With at most 64 possible
// actions it is the k-th clear bit of `tried`; beyond, the smallest t with
// t - #{children with index <= t} = k, reached from t = k by t <- k + #{index <= t}.
__device__ __forceinline__ int mcts_untried(const MctsArgs& A, int64_t i, int node, int count, int K,
                                            uint64_t tried, int k) {
    if (K <= 64) {
        uint64_t open = ~tried;
        for (int q = 0; q < k; ++q) open &= open - 1;
        return __ffsll((unsigned long long)open) - 1;
    }
    int t = k;
    for (;;) {
        int below = 0;
        for (int j = 1; j < count; ++j) {
            const int4 m = A.rec[(int64_t)j * A.n + i];
            below += ((int)((uint32_t)m.x & kMctsNoParent) == node) & (m.y <= t);
        }
        if (k + below == t) return t;
        t = k + below;
    }
}

// The playouts. run() plays from the simulation's ship s under its key, leaves the return in ret
// and answers as rollout_run does: SE_ROLL_RAISED where the decision raises there (sample_type:
// the SE_SAMPLE_* type), SE_ROLL_ATTEMPTS where the playout stopped early with a partial return,
// which marks the decision with the sticky status kPartial.
struct MctsRandomPlayout {  // _rollout (:211-238): rollout_run, the code of se_rollout
    using Args = MctsArgs;
    static constexpr int kPartial = SE_MCTS_CUT;
    static __device__ __forceinline__ int32_t run(const Args& A, const LdsWorld& w, Ship& s, const Key& key,
                                                  double& ret, int& sample_type) {
        int32_t steps;
        return rollout_run(w, s, key, A.max_steps, A.max_attempts, ret, steps, sample_type);
    }
};

struct MctsNavArgs : MctsArgs {  // max_attempts is not read
    NavTables tab;
    double refuel_below;
    int32_t load;
};

struct MctsNavPlayout {  // the navigator for max_steps positions: never raises, never cut
    using Args = MctsNavArgs;
    static constexpr int kPartial = SE_MCTS_STUCK;
    static __device__ __forceinline__ int32_t run(const Args& A, const LdsWorld& w, Ship& s, const Key& key,
                                                  double& ret, int&) {
        return nav_playout(w, A.tab, s, key, A.max_steps, A.refuel_below, A.load, ret) ? SE_ROLL_MAX_STEPS
                                                                                       : SE_ROLL_ATTEMPTS;
    }
};

template <class Playout>
__global__ __launch_bounds__(kMctsBlock) void mcts_kernel(typename Playout::Args A) {
    extern __shared__ uint32_t lds[];
    const LdsWorld w = stage_world(A.world, A.dims, lds);
    const int S = A.sims;
    for (int64_t i = (int64_t)blockIdx.x * kMctsBlock + threadIdx.x; i < A.n;
         i += (int64_t)gridDim.x * kMctsBlock) {
        const Ship s0 = load_ship(A.st, i);
        const int64_t id0 = A.mcts_base + (A.env_base + i) * S;
        const uint32_t root = mcts_pack(kMctsNoParent, s0);  // root = MCTSNode(state) (:253)
        A.rec[i] = make_int4((int)root, 0, 0, 0);
        A.total[i] = 0.0;
        int count = 1, status = SE_MCTS_OK, raised = 0;  // raised: the SE_SAMPLE_* type of the raise
        for (int sim = 0; sim < S && !raised; ++sim) {
            const Key key = env_key(A.seed, id0 + sim);
            Ship s = s0;  // _create_env_copy (:257)
            int node = 0, K;
            uint32_t d = 0, word;
            MctsKids kids;
            bool stop = false;
            // selection (:260-268)
            for (;;) {
                const int4 me = A.rec[(int64_t)node * A.n + i];
                word = (uint32_t)me.x;
                K = mcts_possible(w, word);
                kids = mcts_children(A, i, node, count, A.c, me.z);
                if (stop || kids.nch != K) break;  // done / raised below, or not fully expanded
                if (K == 0) {                      // np.argmax([]) raises (:128)
                    raised = SE_SAMPLE_RAISES;
                    break;
                }
                int ty, va, vb;
                mcts_action(w, word, A.rec[(int64_t)kids.best * A.n + i].y, ty, va, vb);
                node = kids.best;
                const U4 blk = draw(key, d, kSlotMcts);
                const Pending p = drawn_step(w, s, key, d, kSlotMctsB, blk, ty, va, vb);
                ++d;
                stop = (p.e != SE_ERR_OK) | p.dead;
            }
            if (raised) break;
            // expansion (:271-279)
            if (K > kids.nch) {
                const U4 blk = draw(key, d, kSlotMcts);
                const int t = mcts_untried(A, i, node, count, K, kids.tried,
                                           uniform_int(blk.v[0], (uint32_t)(K - kids.nch)));
                int ty, va, vb;
                mcts_action(w, word, t, ty, va, vb);
                const Pending p = drawn_step(w, s, key, d, kSlotMctsB, blk, ty, va, vb);
                if (p.e != SE_ERR_OK) continue;  // except Exception: continue (:278)
                const int64_t at = (int64_t)count * A.n + i;
                A.rec[at] = make_int4((int)mcts_pack((uint32_t)node, s), t, 0, 0);
                A.total[at] = p.r;  // child.total_reward = reward (:145)
                node = count++;
            }
            // simulation (:282): _rollout sits outside any try
            double ret;
            int sample_type;
            const int32_t rs = Playout::run(A, w, s, key, ret, sample_type);
            if (rs == SE_ROLL_RAISED) {
                raised = sample_type;
                break;
            }
            if (rs == SE_ROLL_ATTEMPTS) status = Playout::kPartial;
            // backpropagation (:149-159)
            for (;;) {
                const int64_t at = (int64_t)node * A.n + i;
                int4 me = A.rec[at];
                me.z += 1;
                A.rec[at] = me;
                A.total[at] += ret;
                if (node == 0) break;
                node = (int)((uint32_t)me.x & kMctsNoParent);
            }
        }
        int ty = raised, va = 0, vb = 0;
        if (!raised) {
            const MctsKids kids = mcts_children(A, i, 0, count, 0.0, A.rec[i].z);
            if (kids.nch > 0) {  // root.best_child(c_param=0) (:288-290)
                mcts_action(w, root, A.rec[(int64_t)kids.best * A.n + i].y, ty, va, vb);
            } else {  // self.env.sample_action() (:292)
                const U4 blk = draw(env_key(A.seed, id0), 0xffffffffu, kSlotMcts);
                sample_action(w, s0, blk.v[0], ty, va, vb);
                raised = ty < 0 ? ty : 0;
            }
        }
        if (raised) status = raised == SE_SAMPLE_NO_OTHER_PORT ? SE_MCTS_NEVER_RETURNS : SE_MCTS_RAISED;
        A.type[i] = ty;
        A.a[i] = va;
        A.b[i] = vb;
        A.status[i] = status;
        if (A.tree) {
            se_mcts_node* out = A.tree + i * (S + 1);
            for (int j = 0; j < count; ++j) {
                const int64_t at = (int64_t)j * A.n + i;
                const int4 me = A.rec[at];
                se_mcts_node nd{-1, 0, 0, 0, me.z, 0, A.total[at]};
                if (j > 0) {
                    nd.parent = (int32_t)((uint32_t)me.x & kMctsNoParent);
                    mcts_action(w, (uint32_t)A.rec[(int64_t)nd.parent * A.n + i].x, me.y, nd.type, nd.a, nd.b);
                }
                out[j] = nd;
            }
            A.tree_count[i] = count;
        }
    }
}

}  // namespace

struct se_mcts {
    se_env* env = nullptr;  // must outlive the handle (destroy the handle first)
    int device = 0;
    int32_t max_sims = 0;
    int64_t n = 0;              // envs the scratch was sized for
    double* d_log = nullptr;    // [max_sims + 1]
    uint8_t* d_tree = nullptr;  // rec and total, [max_sims + 1][n] each
};

extern "C" {

int se_mcts_create(se_mcts** out, se_env* env, int32_t max_simulations) {
    if (!out) return fail(SE_EINVAL, "null out");
    *out = nullptr;
    int rc = check_ready(env);
    if (rc) return rc;
    if (max_simulations < 1 || max_simulations > kMctsMaxSims)
        return fail(SE_EINVAL, "max_simulations must be in 1..256");
    DeviceGuard g(env->device);
    se_mcts* m = new se_mcts;
    m->env = env;
    m->device = env->device;
    m->max_sims = max_simulations;
    m->n = env->n;
    // np.log(parent.visits) (:125) from the host's C library: visits <= simulations
    std::vector<double> tab((size_t)max_simulations + 1, 0.0);
    for (int v = 1; v <= max_simulations; ++v) tab[v] = log((double)v);
    hipError_t e = hipMalloc(&m->d_log, tab.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(m->d_log, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice);
    // a 16-byte record (node word, action index, visits) and total_reward (8) per node and env
    if (e == hipSuccess && m->n > 0) e = hipMalloc(&m->d_tree, (size_t)(max_simulations + 1) * (size_t)m->n * 24);
    if (e != hipSuccess) {
        se_mcts_destroy(m);
        return fail(SE_EHIP, std::string("se_mcts_create: ") + hipGetErrorString(e));
    }
    *out = m;
    return SE_OK;
}

}  // extern "C"

namespace {

// What both entry points check of their arguments, none of it the env's or a handle's state.
int mcts_check(const se_mcts* m, int32_t simulations, double c_param, int32_t max_rollout_steps,
               int32_t max_attempts, int64_t mcts_base, const int32_t* type, const int32_t* a, const int32_t* b,
               const int32_t* status, const se_mcts_node* tree, const int32_t* tree_count) {
    const se_env* env = m->env;
    if (env->n != m->n) return fail(SE_EINVAL, "the env's size changed since se_mcts_create");
    if (simulations < 1 || simulations > m->max_sims)
        return fail(SE_EINVAL, "simulations must be in 1..max_simulations");
    if (!(c_param == c_param)) return fail(SE_EINVAL, "c_param is NaN");
    if (max_rollout_steps < 0 || max_attempts < 0 || mcts_base < 0)
        return fail(SE_EINVAL, "max_rollout_steps, max_attempts and mcts_base must be >= 0");
    int64_t ids, last;  // ids run up to mcts_base + (env_id_base + n) * simulations - 1
    if (__builtin_add_overflow(env->env_base, env->n, &ids) || __builtin_mul_overflow(ids, (int64_t)simulations, &ids) ||
        __builtin_add_overflow(ids, mcts_base, &last))
        return fail(SE_EINVAL, "mcts_base + (env_id_base + n) * simulations overflows int64");
    if (env->n == 0) return SE_OK;
    if (!type || !a || !b || !status) return fail(SE_EINVAL, "null output pointer");
    if ((tree == nullptr) != (tree_count == nullptr)) return fail(SE_EINVAL, "tree and tree_count go together");
    if (!aligned16(type) || !aligned16(a) || !aligned16(b) || !aligned16(status) || !aligned16(tree) ||
        !aligned16(tree_count))
        return fail(SE_EINVAL, "outputs must be 16-byte aligned");
    return SE_OK;
}

// One launch of the decision kernel with playout Playout; `extra` fills what its Args add.
template <class Playout, class Extra>
int mcts_launch(se_mcts* m, int32_t simulations, double c_param, int32_t max_rollout_steps, int32_t max_attempts,
                int64_t mcts_base, int32_t* type, int32_t* a, int32_t* b, int32_t* status, se_mcts_node* tree,
                int32_t* tree_count, void* stream, Extra extra) {
    se_env* env = m->env;
    DeviceGuard g(env->device);
    size_t lds;
    const int rc = world_lds<mcts_kernel<Playout>>(env, lds);
    if (rc) return rc;
    const size_t nodes = (size_t)(m->max_sims + 1) * (size_t)m->n;
    typename Playout::Args A{};
    static_cast<EnvArgs&>(A) = env_args(env);
    A.mcts_base = mcts_base;
    A.sims = simulations;
    A.max_steps = max_rollout_steps;
    A.max_attempts = max_attempts;
    A.c = c_param;
    A.logtab = m->d_log;
    A.rec = reinterpret_cast<int4*>(m->d_tree);
    A.total = reinterpret_cast<double*>(m->d_tree + 16 * nodes);
    A.type = type;
    A.a = a;
    A.b = b;
    A.status = status;
    A.tree = tree;
    A.tree_count = tree_count;
    extra(A);
    const int64_t blocks = (env->n + kMctsBlock - 1) / kMctsBlock;
    mcts_kernel<Playout><<<(int)std::min<int64_t>(blocks, kMctsMaxBlocks), kMctsBlock, lds, (hipStream_t)stream>>>(A);
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

}  // namespace

extern "C" {

int se_mcts_choose(se_mcts* m, int32_t simulations, double c_param, int32_t max_rollout_steps,
                   int32_t max_attempts, int64_t mcts_base, int32_t* type, int32_t* a, int32_t* b,
                   int32_t* status, se_mcts_node* tree, int32_t* tree_count, void* stream) {
    if (!m) return fail(SE_EINVAL, "null mcts handle");
    int rc = check_ready(m->env);
    if (rc) return rc;
    rc = mcts_check(m, simulations, c_param, max_rollout_steps, max_attempts, mcts_base, type, a, b, status, tree,
                    tree_count);
    if (rc || m->env->n == 0) return rc;
    return mcts_launch<MctsRandomPlayout>(m, simulations, c_param, max_rollout_steps, max_attempts, mcts_base, type,
                                          a, b, status, tree, tree_count, stream, [](MctsArgs&) {});
}

int se_mcts_choose_nav(se_mcts* m, se_nav* nav, double refuel_below, int32_t load, int32_t simulations,
                       double c_param, int32_t max_rollout_steps, int64_t mcts_base, int32_t* type, int32_t* a,
                       int32_t* b, int32_t* status, se_mcts_node* tree, int32_t* tree_count, void* stream) {
    // the arguments first: misuse is reported whatever the handles' state
    if (!m) return fail(SE_EINVAL, "null mcts handle");
    if (!nav) return fail(SE_EINVAL, "null nav handle");
    if (load < 0) return fail(SE_EINVAL, "load must be >= 0");
    int rc = mcts_check(m, simulations, c_param, max_rollout_steps, 0, mcts_base, type, a, b, status, tree,
                        tree_count);
    if (rc) return rc;
    if (nav->env != m->env) return fail(SE_EINVAL, "the nav handle was made on another env");
    rc = nav_ready(nav);
    if (rc || m->env->n == 0) return rc;
    const NavTables tab{nav->d_field, nav->d_dir};
    return mcts_launch<MctsNavPlayout>(m, simulations, c_param, max_rollout_steps, 0, mcts_base, type, a, b, status,
                                       tree, tree_count, stream, [&](MctsNavArgs& A) {
                                           A.tab = tab;
                                           A.refuel_below = refuel_below;
                                           A.load = load;
                                       });
}

int se_mcts_destroy(se_mcts* m) {
    if (!m) return SE_OK;
    DeviceGuard g(m->device);
    const hipError_t e = device_free({m->d_log, m->d_tree});
    delete m;
    return e == hipSuccess ? SE_OK : fail(SE_EHIP, std::string("hipFree: ") + hipGetErrorString(e));
}

}  // extern "C"
