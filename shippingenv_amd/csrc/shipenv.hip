// shipenv.hip — MI355X (gfx950) batched ShippingEnv: step / reset / observe kernels
// and the C-ABI of include/shipenv.h.
//
// What one step does per environment is shipping/environment.py:359-376 (step)
// and :273-339 (_move_ship) of the reference; DESIGN.md walks through the
// mapping. The shape of the work is what drives the design:
//   * the path is HBM-streaming integer/f64 work, ~0 useful FLOPs: no MFMA;
//   * state is SoA with narrow fields (u8 positions/indices, i32 cargo,
//     f64 fuel) so each field of 4 consecutive envs is one 4-/16-byte lane
//     access: every wave instruction is a fully coalesced 256 B - 1 KiB access;
//   * the static world (ground bitmap, port bitmap, ports table) is staged once
//     per workgroup into LDS; the per-env map lookups are LDS reads;
//   * RNG is counter-based Philox keyed by (seed, global env id): 0 bytes of RNG
//     state in HBM and shard-invariant results;
//   * auto-reset compacts finished envs into a done list with a wave ballot
//     prefix into per-(iteration, wave) segments (no atomics, no barrier), and
//     reduces episode statistics per wave into a fixed slab (deterministic sums,
//     no float atomics).
//
// Built with -ffp-contract=off: the reference's f64 arithmetic (CPython float,
// np.sqrt) is unfused, and an FMA in -0.1 + 0.2*u changes fuel bits.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/shipenv.h"
#include "navfield.h"
#include "philox.h"
#include "step_lean.h"

#ifndef SHIPENV_TRACE
#define SHIPENV_TRACE 0  // 1 = diagnostic build: per-wave phase timestamps (tools/archive/wave_trace.py)
#endif

using namespace shipenv;

namespace {

constexpr int kBlock = 256;       // 4 waves
constexpr int kStepBlock = 256;  // step kernel workgroup (one LDS world copy each)
constexpr int kEnvsPerThread = 4; // one 4-byte / 16-byte lane access per field
constexpr int kMaxBlocks = 2048;  // 256 CUs x 8; grid-stride beyond
// step kernel default workgroup cap (SHIPENV_STEP_BLOCKS overrides): one group of 4 envs per
// thread up to 2^25 envs. Measured against 2048 (iters = 8 at 2^24; tools/archive/blk_sweep.sh,
// profiles/r02h/blk_sweep): 2^24 129 -> 123 us, 2^25 293 -> 253 us, config 4 at 2^24
// 200 -> 182 us; 2^20 (grid 1024 either way) unchanged
constexpr int kStepBlocks = 32768;

// se_tape.used bits (replay): which of the reference's draws this step consumed
constexpr uint32_t kUsedFuelGate = SE_USED_FUEL_GATE, kUsedLossType = SE_USED_LOSS_TYPE,
                   kUsedBeta = SE_USED_BETA, kUsedArrive = SE_USED_ARRIVE, kUsedMoved = SE_USED_MOVED;

// reference constants, shipping/environment.py:8-26
constexpr double kFuelInit = 200.0;
constexpr double kMaxCargo = 50.0;

// The device side, in fragments of this translation unit (DESIGN.md has the file map). Each
// is included where its text stood, inside this anonymous namespace, and uses the ones above
// it: the order is the order of definition and is part of the tuning, so it does not change.
#include "world.h"        // world image layout, WorldDims, LdsWorld, LDS staging
#include "env_core.h"     // the per-env step core (host + device): Ship, env_begin/env_finish, replay_env
#include "step_io.h"      // StepRecord, StepArgs, streaming group loads and stores, Group
#include "step_group.h"   // step_group: the typed and replay step of one group
#include "step_agent.h"   // step_group_agent: the packed agent-index step of one group
#include "step_kernel.h"  // wave reductions, done-list compaction, step_kernel, step_tail_kernel
#include "step_seq.h"     // step_group_state, step_seq_kernel, step_tail_seq_kernel
#include "views.h"        // done-list copy, reset, observe, valid masks, gen_actions
#include "rollout.h"      // random policy, rollouts, episode statistics
#include "episode.h"      // the rollout scaffold: the lane, the tally and the store of its results
#include "plan.h"         // scripted rollouts: the scaffold with its actions read from memory
}  // namespace

// ====================================================================== host side
struct se_env {
    int device = 0;
    int64_t n = 0, env_base = 0;
    WorldDims dims{};
    uint64_t seed = 0;
    uint32_t flags = 0;
    uint64_t step_t = 0, epoch = 0;
    std::vector<uint8_t> water;  // H*W, 0 = ground
    std::vector<int32_t> port_x, port_y;  // the ports of the uploaded world (se_nav builds its tables from them)
    uint32_t* d_world = nullptr;
    int64_t seg = 0;    // done-list segment stride (records per wave-iteration: 256)
    int64_t iters = 1;  // groups per thread of the step kernel
    size_t world_cap = 0;  // bytes allocated
    uint64_t world_version = 0;  // bumped by every world upload (se_qnet folds the ports)
    int32_t cmax = 0, fmax = 0;  // largest TAKE_CARGO / TAKE_FUEL amount any port allows (se_qnet)
    int32_t stock_cargo_max = 0;  // largest port_cargo (se_sarsa: sample_action takes up to the whole stock)
    se_state st{};
    bool bound = false;
    double* d_slab = nullptr;       // [nslab][4]
    int32_t* d_offsets = nullptr;   // [nseg] se_done_compact scratch
    int grid = 0;
    int64_t nseg = 0;   // done-list segments: one per (iteration, wave) of the step kernel
    int64_t nslab = 0;  // stats slab entries: one per step-kernel wave
    uint8_t* d_mask_tmpl = nullptr;  // se_valid_mask's row templates (mask_tmpl_kernel), lazily built
    size_t mask_tmpl_cap = 0;
    uint64_t mask_tmpl_version = 0;  // world_version they were built from (0: none)
    int mask_ntmpl = 0;              // 1 + P + sum_p |ports on p's cell| (upload_world)
    bool mask_tiled = false;         // SHIPENV_MASK_TILED=1 at se_create: the round-4 tiled kernel
    int32_t done_pad = 1;   // done-list records padded to runs of this many (done_pad_records)
    bool nt_loads = false;  // nontemporal state loads in the step kernel (step_nt_loads)
    bool seq_fuse = true;   // se_step_seq without auto-reset: one launch per run (SHIPENV_SEQ_FUSE=0: one per step)
    int32_t seq_max_steps = 1024;  // steps of one fused launch at most (seq_max_steps)
    bool seq_gate_pool = true;  // the fused launch draws GATE through the wave's pool (SHIPENV_SEQ_GATE_POOL=0: draw2)
    bool seq_ring = true;       // the fused launch's regular waves step on the bordered cell table (SHIPENV_SEQ_RING=0: none do)
    bool seq_screen = true;     // the GATE pool's refill screens its words, cold steps test no gate (SHIPENV_SEQ_SCREEN=0: every step does)
    bool ports_distinct = false;  // all ports lie on distinct cells (build_world_image): with two or more, the fused launch may test arrivals by the cell code
};

// A host-resident world (se_host_*): no device, no HIP call. It steps envs whose SoA
// state lives in host memory with the kernels' own per-env code (replay_env).
struct se_host {
    WorldDims dims{};
    std::vector<uint8_t> water;  // H*W, 0 = ground
    std::vector<uint32_t> img;   // the world image, as staged into LDS on the device
};

namespace {

#include "host.h"  // fail, HIP_TRY, DeviceGuard, device blocks, the LDS opt-in, check_ready

// ---------------------------------------------------------------- launch-time switches
// SHIPENV_STEP_BLOCKS, _DONE_PAD, _NT_LOADS, _SEQ_MAX_STEPS, _SEQ_FUSE, _SEQ_GATE_POOL, _SEQ_RING,
// _SEQ_SCREEN and _MASK_TILED: se_create resolves all nine, once, into the se_env, and a launch
// reads no environment variable.

// Workgroup cap of the step kernel: each thread then walks ceil(groups / (cap*256))
// groups, loading the next group after storing the current one.
int step_block_cap() {
    const char* v = getenv("SHIPENV_STEP_BLOCKS");
    const int c = v ? atoi(v) : 0;
    return c > 0 ? c : kStepBlocks;
}

// Nontemporal state loads for the kernels without auto-reset while one step's traffic
// (~42 B per env) stays inside or near the 256 MiB Infinity Cache. Forced on vs off at
// the 32768-workgroup cap (profiles/r02h/nt_sweep, two runs each): config 3 at 2^20
// 8.5-8.8 vs 9.1-9.2 us, at 2^24 131-134 vs 123 us. The auto-reset kernels are faster
// without them up to 2^21 envs (config 4 at 2^20 11.6 vs 12.5 us; the training loop's step
// + record 16.0-16.3 vs 17.5-17.9 us) and with them beyond (below).
// The done list's records padded to whole 128-B lines (wave_compact) once the step's traffic
// is beyond the Infinity Cache: config 4 at 2^24 -2.7 us per step (median of five alternating
// rounds), at 2^20 +0.17 us (profiles/r04/ab_donepad.jsonl). SHIPENV_DONE_PAD overrides.
// Both settings are resolved once, by se_create (se_env::done_pad / nt_loads): a launch
// reads no environment variable, and the layout cannot change between two steps.
int32_t done_pad_records(const se_env* env) {
    const char* v = getenv("SHIPENV_DONE_PAD");
    if (v) return atoi(v) == 0 ? 1 : 8;
    return env->n > (int64_t)1 << 23 ? 8 : 1;
}

// Round 5 (episode-start stamps): the auto-reset kernel's few scattered stamp accesses per
// wave are cheap while the state streams do not evict them from the Infinity Cache, which
// the streams' nontemporal loads achieve. Config 4, alternating (profiles/r05/nt_sweep_c4.jsonl):
// 2^20 11.6 (temporal) vs 12.5 us (nontemporal), 2^22 43.6 vs 43.3, 2^23 83.0 vs 80.4,
// 2^24 173.4 vs 157.3, 2^25 339.5 vs 310.6; so nontemporal above 2^21 envs.
bool step_nt_loads(const se_env* env) {
    const char* v = getenv("SHIPENV_NT_LOADS");
    if (v) return atoi(v) != 0;
    if (env->flags & SE_FLAG_AUTO_RESET) return env->n > (int64_t)1 << 21;
    return env->n <= (int64_t)1 << 23;
}

// se_step_seq's fused launches (step_seq_kernel) hold the queue for their whole run: about
// 3.5 ms for 1024 steps at 2^20 envs. A longer sequence goes out as several launches of at
// most this many steps. SHIPENV_SEQ_MAX_STEPS overrides; SHIPENV_SEQ_FUSE=0 issues one
// step_kernel<..., kSeq> launch per step instead (the A/B baseline). Both are resolved
// once, by se_create.
constexpr int32_t kSeqMaxSteps = 1024;
int32_t seq_max_steps() {
    const char* v = getenv("SHIPENV_SEQ_MAX_STEPS");
    const int c = v ? atoi(v) : 0;
    return c > 0 ? c : kSeqMaxSteps;
}
bool seq_fuse() {
    const char* v = getenv("SHIPENV_SEQ_FUSE");
    return !v || atoi(v) != 0;
}

// SHIPENV_SEQ_GATE_POOL=0: the fused launch's state-only steps draw FUEL and GATE together every
// step (draw2) instead of taking GATE from the wave's pool (step_seq.h): the same-library control
// of the pool's measurements and tests. Results are the same bits either way.
bool seq_gate_pool() {
    const char* v = getenv("SHIPENV_SEQ_GATE_POOL");
    return !v || atoi(v) != 0;
}

// SHIPENV_SEQ_RING=0: the fused launch carries no bordered cell table (step_lean.h), so every wave
// runs the general state-only step and draws directly (step_seq.h): the same-library control of
// the table's measurements and tests. Results are the same bits either way.
bool seq_ring() {
    const char* v = getenv("SHIPENV_SEQ_RING");
    return !v || atoi(v) != 0;
}

// SHIPENV_SEQ_SCREEN=0: every step of a pooled window counts as hot (the launch's screen_all is
// all-ones, OR-ed into each window's screen), so every step reads its pool entry and tests the
// gate, as before the screen (step_seq.h): the same-library control of the screen's measurements
// and tests. Results are the same bits either way.
bool seq_screen() {
    const char* v = getenv("SHIPENV_SEQ_SCREEN");
    return !v || atoi(v) != 0;
}

// SHIPENV_MASK_TILED=1: se_valid_mask takes the round-4 tiled kernel (valid_mask_tiled_kernel)
// where it would take the row templates; tests reach that kernel at small P this way.
bool mask_tiled() {
    const char* v = getenv("SHIPENV_MASK_TILED");
    return v && atoi(v) != 0;
}

// The world image (layout above WorldDims, world.h) of an H x W map and P ports, built on the
// host: uploaded by se_create / se_set_ports, kept as is by the host handles. *distinct: do all
// ports lie on distinct cells, so that a cell's code names the one port on it (step_lean.h).
int build_world_image(int H, int W, const std::vector<uint8_t>& water, int32_t P, const int32_t* px,
                      const int32_t* py, const int32_t* pf, const int32_t* pc, WorldDims& dims,
                      std::vector<uint32_t>& img, bool* distinct = nullptr) {
    if (P < 0 || P > SE_MAX_PORTS) return fail(SE_EINVAL, "P must be in [0, 254]");
    for (int i = 0; i < P; ++i) {
        if (px[i] < 0 || px[i] >= H || py[i] < 0 || py[i] >= W)
            return fail(SE_EINVAL, "Coordinates not within map");  // add_port, environment.py:59-60
        if (pf[i] < 0 || pc[i] < 0) return fail(SE_EINVAL, "port stocks must be >= 0");
    }
    const int cw = (H * W + 15) / 16 * 4;  // cell-code bytes in whole 16-byte units
    WorldDims d{H, W, P, cw};
    img.assign((size_t)d.padded(), 0u);
    uint8_t* cell = reinterpret_cast<uint8_t*>(img.data());
    for (int c = 0; c < H * W; ++c) cell[c] = water[c] ? 0 : (uint8_t)kCellGround;
    for (int i = P - 1; i >= 0; --i)  // Entity.PORT (:65); the first port on a cell wins
        cell[(size_t)px[i] * W + py[i]] = (uint8_t)(i + 1);
    for (int i = 0; i < P; ++i) {
        img[d.pos() + i] = (uint32_t)px[i] | ((uint32_t)py[i] << 16);
        img[d.stk() + 2 * i] = (uint32_t)pf[i];
        img[d.stk() + 2 * i + 1] = (uint32_t)pc[i];
    }
    // normalize(cargo, 50, 0) = cargo / 50 (util.py:6-8): Python's int / int true
    // division is the correctly rounded quotient, which IEEE f64 division gives here.
    for (int c = 0; c < 50; ++c) {
        const double q = (double)c / kMaxCargo;
        memcpy(&img[d.frac() + 2 * c], &q, sizeof q);
    }
    // exact product, q < 1; cargo >= 50: random() < 1 <= cargo / 50 (step_lean.h)
    for (int c = 0; c <= 50; ++c) img[d.gate() + c] = gate_thr_entry(c, kMaxCargo);
    // N, E, S, W as packed 16-bit (dx, dy) (shipping/type.py:8-16)
    const int mdx[4] = {0, -1, 0, 1}, mdy[4] = {-1, 0, 1, 0};
    for (int k = 0; k < 4; ++k)
        img[d.moves() + k] = ((uint32_t)mdx[k] & 0xffffu) | (((uint32_t)mdy[k] & 0xffffu) << 16);
    // step rewards before cargo loss / arrival, added in the reference's order:
    // out of fuel (:288-290), ground (:293-294) or fuel + water (:296-300), closer (:307-315)
    double rtab[10];
    for (int k = 0; k < 8; ++k) {
        double r = 0.0;
        if (k & 4) r += -10.0;
        if (k & 2) {
            r += -5.0;
        } else {
            r += -0.0001;
            r += -1.0;
        }
        r += (k & 1) ? 2.0 : -2.0;
        rtab[k] = r;
    }
    rtab[8] = 0.05;  // TAKE_FUEL / TAKE_CARGO (:349, :357)
    rtab[9] = 0.0;
    memcpy(&img[d.rtab()], rtab, sizeof rtab);
    dims = d;
    if (distinct) *distinct = ports_on_distinct_cells(P, px, py);
    return SE_OK;
}

int upload_world(se_env* env, int32_t P, const int32_t* px, const int32_t* py, const int32_t* pf,
                 const int32_t* pc) {
    WorldDims d{};
    std::vector<uint32_t> img;
    bool distinct = false;
    int rc = build_world_image(env->dims.H, env->dims.W, env->water, P, px, py, pf, pc, d, img, &distinct);
    if (rc) return rc;
    // the bordered cell table of the fused step sequence's regular waves (step_lean.h) follows
    // the image; no other kernel reads past the image
    std::vector<uint8_t> ring(ring_table_bytes(d.H, d.W));
    ring_table_build(d.H, d.W, reinterpret_cast<const uint8_t*>(img.data()), ring.data());
    rc = device_reserve(env->d_world, env->world_cap, (size_t)d.padded() * 4 + ring.size());
    if (rc) return rc;
    HIP_TRY(hipMemcpy(env->d_world, img.data(), (size_t)d.padded() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(env->d_world + d.padded(), ring.data(), ring.size(), hipMemcpyHostToDevice));
    env->dims = d;
    env->ports_distinct = distinct;
    env->port_x.assign(px, px + P);
    env->port_y.assign(py, py + P);
    env->cmax = env->fmax = env->stock_cargo_max = 0;
    for (int i = 0; i < P; ++i) {  // amounts 1..49 / 1..199 exist (utils/preprocessing.py:93-108)
        env->cmax = std::max(env->cmax, std::min(pc[i], 49));
        env->fmax = std::max(env->fmax, std::min(pf[i], 199));
        env->stock_cargo_max = std::max(env->stock_cargo_max, pc[i]);
    }
    env->world_version += 1;
    env->mask_ntmpl = 1 + P;  // se_valid_mask's row templates (mask_tmpl_kernel)
    for (int p = 0; p < P; ++p)
        for (int q = 0; q < P; ++q) env->mask_ntmpl += (px[p] == px[q] && py[p] == py[q]) ? 1 : 0;
    return SE_OK;
}

// The step kernels a launch chooses among, as tables. A row is written step_row<flags>() /
// tail_row<flags>(): its flags appear once and give both the key the selection matches and the
// kernel's template arguments (in the kernels' own order: kTyped, kReplay, kAuto, kNt, kRec,
// kSeq), so no row can send a flag combination to another instantiation. The rows are all the
// instantiations there are: a combination without a row has no kernel and is an error.
typedef void (*StepFn)(StepArgs);
struct StepRow {
    uint32_t key;
    StepFn fn;
};
constexpr uint32_t step_key(bool typed, bool replay, bool autoreset, bool nt = false, bool rec = false, bool seq = false) {
    return typed | replay << 1 | autoreset << 2 | nt << 3 | rec << 4 | seq << 5;
}
template <bool... kFlags>
constexpr StepRow step_row() {
    return {step_key(kFlags...), step_kernel<kFlags...>};
}
template <bool... kFlags>
constexpr StepRow tail_row() {
    return {step_key(kFlags...), step_tail_kernel<kFlags...>};
}
constexpr StepRow kStepKernels[] = {
    step_row<false, false, false>(), step_row<false, false, false, true>(),  // se_step; with nontemporal loads
    step_row<false, false, true>(), step_row<false, false, true, true>(),    // ... with auto-reset
    step_row<false, false, false, false, false, true>(),  // se_step_seq's launch per step (SHIPENV_SEQ_FUSE=0)
    step_row<false, false, false, true, false, true>(),
    step_row<false, false, true, false, true>(), step_row<false, false, true, true, true>(),  // se_step_record
    step_row<false, true, false>(), step_row<true, true, false>(),  // se_step_agent_replay, se_step_replay
    step_row<true, false, false>(), step_row<true, false, true>(),  // se_step_typed; with auto-reset
};
constexpr StepRow kStepTailKernels[] = {
    tail_row<false, false, false>(), tail_row<false, false, true>(), tail_row<false, true, false>(),
    tail_row<true, true, false>(),   tail_row<true, false, false>(), tail_row<true, false, true>(),
};

template <size_t kRows>
StepFn find_kernel(const StepRow (&rows)[kRows], uint32_t key) {
    for (const StepRow& r : rows)
        if (r.key == key) return r.fn;
    return nullptr;
}

// What every step launch passes: the world, the batch, the draw key, the bound state and the
// action row. launch_step adds the typed, tape, done-list, statistics and record fields.
StepArgs step_args(const se_env* env, const int32_t* act) {
    StepArgs A{};
    A.world = env->d_world;
    A.dims = env->dims;
    A.n = env->n;
    A.env_base = env->env_base;
    A.seed = env->seed;
    A.t = (uint32_t)env->step_t;
    A.st = env->st;
    A.act = act;
    A.iters = env->iters;
    return A;
}

int launch_step(se_env* env, bool typed, bool replay, const int32_t* act, const int32_t* a,
                const int32_t* b, se_tape* tape, void* stream, const StepRecord* rec = nullptr,
                bool seq = false) {
    int rc = check_ready(env);
    if (rc) return rc;
    if (env->n > 0 && (!act || (typed && (!a || !b)) || (replay && !tape)))  // n = 0: an empty batch
        return fail(SE_EINVAL, "null action/tape pointer");
    if (!aligned16(act) || (typed && (!aligned16(a) || !aligned16(b))))
        return fail(SE_EINVAL, "action buffers must be 16-byte aligned");
    const bool autoreset = (env->flags & SE_FLAG_AUTO_RESET) && !replay;
    if (autoreset && env->dims.P < 2) return fail(SE_EINVAL, "auto-reset needs at least two ports");
    DeviceGuard g(env->device);
    StepArgs A = step_args(env, act);
    A.act_a = a;
    A.act_b = b;
    A.tape = tape;
    // done lists double-buffered by step parity: the list of step t-1 stays
    // readable while step t runs; every block rewrites its own count each step.
    if (autoreset) {
        const size_t par = (size_t)(env->step_t & 1u);
        A.done_recs = env->st.done_recs + par * (size_t)env->nseg * (size_t)env->seg;
        A.done_count = env->st.done_count + par * (size_t)env->nseg;
    }
    A.seg = env->seg;
    A.done_pad = env->done_pad;
    A.slab = env->d_slab;
    if (rec) A.rec = *rec;  // se_step_record: the caller checked agent actions, auto-reset, n % 4 == 0, n > 0
    // only the packed agent step (agent actions, Philox draws) has nontemporal-load variants, and
    // only it, without auto-reset, has se_step_seq's; a partial last group has neither
    const bool agent = !typed && !replay;
    const StepFn full = find_kernel(kStepKernels, step_key(typed, replay, autoreset, agent && env->nt_loads,
                                                           rec != nullptr, agent && !autoreset && seq));
    const StepFn tail = find_kernel(kStepTailKernels, step_key(typed, replay, autoreset));
    if (!full || !tail) return fail(SE_EINVAL, "no step kernel for this kind of step");
    const hipStream_t s = (hipStream_t)stream;
    if (env->n >= kEnvsPerThread) {  // at least one full group (step_kernel's first load assumes it)
        full<<<env->grid, kStepBlock, lds_bytes(env), s>>>(A);
        HIP_TRY(hipGetLastError());
    }
    if (env->n & 3) {
        tail<<<1, 64, 0, s>>>(A);
        HIP_TRY(hipGetLastError());
    }
    if (!replay) env->step_t += 1;
    return SE_OK;
}

// `steps` > 0 consecutive agent steps without auto-reset as one fused launch (plus the
// partial last group's), rows `ld` apart from act; the caller checked the env and the stride.
int launch_step_seq(se_env* env, const int32_t* act, int64_t ld, int32_t steps, void* stream) {
    if (!act) return fail(SE_EINVAL, "null action/tape pointer");
    if (!aligned16(act)) return fail(SE_EINVAL, "action buffers must be 16-byte aligned");
    DeviceGuard g(env->device);
    const StepArgs A = step_args(env, act);
    const hipStream_t s = (hipStream_t)stream;
    if (env->n >= kEnvsPerThread) {  // at least one full group (the kernel's first load assumes it)
        // the image, then stock_by_code's table, then the waves' GATE pools. A world whose image
        // leaves no room for the pools under the 64 KiB a launch can ask for draws directly.
        const size_t base = lds_bytes(env) + kStockByCodeBytes;
        const bool pool = env->seq_gate_pool && base + kGatePoolBytes <= kLdsDefault;
        // then the bordered cell table, where the world has one and four workgroups still share a CU
        const size_t without = base + (pool ? kGatePoolBytes : 0);
        // (with the move deltas behind it: kRingDeltaBytes, whichever form the launch's regular waves take)
        const uint32_t ring = env->seq_ring && ring_table_fits(env->dims.H, env->dims.W, env->dims.P, without + kSeqDeltaBytes)
                                  ? ring_table_bytes(env->dims.H, env->dims.W) : 0u;
        const size_t lds = without + ring + (ring ? kSeqDeltaBytes : 0);
        // the carried cell address: a launch with the table whose move deltas are bytes
        const bool addr = SHIPENV_SEQ_CELL_ADDR && ring != 0 && ring_byte_deltas(env->dims.W);
        auto kernel = pool ? (env->nt_loads ? step_seq_kernel<true, true, false> : step_seq_kernel<false, true, false>)
                           : (env->nt_loads ? step_seq_kernel<true, false, false> : step_seq_kernel<false, false, false>);
#if SHIPENV_SEQ_CELL_ADDR
        if (addr)
            kernel = pool ? (env->nt_loads ? step_seq_kernel<true, true, true> : step_seq_kernel<false, true, true>)
                          : (env->nt_loads ? step_seq_kernel<true, false, true> : step_seq_kernel<false, false, true>);
#endif
        kernel<<<env->grid, kStepBlock, lds, s>>>(A, steps, ld, ring | (arrive_by_code_allowed(env->dims.P, env->ports_distinct) ? kSeqDistinctPorts : 0u), env->seq_screen ? 0u : ~0u,
                                                  addr ? ring_unindex_mul(env->dims.W) : 0u);
        HIP_TRY(hipGetLastError());
    }
    if (env->n & 3) {
        step_tail_seq_kernel<<<1, 64, 0, s>>>(A, steps, ld);
        HIP_TRY(hipGetLastError());
    }
    env->step_t += (uint64_t)steps;
    return SE_OK;
}

// reset_kernel over the masked envs (all without a mask): to the given origin / dest, or with
// both null to ports drawn under the current epoch. The caller checked the env and its
// arguments, and bumps the epoch where it drew (se_reset).
int launch_reset(se_env* env, const uint8_t* mask, const int32_t* origin, const int32_t* dest, void* stream) {
    if (env->n == 0) return SE_OK;
    DeviceGuard g(env->device);
    const ResetArgs A{env->d_world, env->dims, env->n, env->env_base, env->seed,
                      (uint32_t)env->epoch, (uint32_t)env->step_t, env->st, mask, origin, dest};
    reset_kernel<<<grid_for(env->n), kBlock, 0, (hipStream_t)stream>>>(A);
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

}  // namespace

// error text for se_last_error from the host-only sources (mapload.cpp)
void shipenv_set_error(const std::string& msg) { g_err = msg; }

extern "C" {

#if SHIPENV_TRACE
extern "C" int se_trace_read(void* host, size_t bytes) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_trace), bytes) == hipSuccess ? 0 : -1;
}
#endif

int se_abi_version(void) { return SHIPENV_ABI_VERSION; }

const char* se_last_error(void) { return g_err.c_str(); }

int se_create(se_env** out, int device, int64_t n, int64_t env_id_base, int32_t H, int32_t W,
              const uint8_t* water, int32_t P, const int32_t* port_x, const int32_t* port_y,
              const int32_t* port_fuel, const int32_t* port_cargo, uint64_t seed, uint32_t flags) {
    if (!out) return fail(SE_EINVAL, "null out");
    *out = nullptr;
    if (n < 0) return fail(SE_EINVAL, "n must be >= 0");
    if (env_id_base < 0 || (env_id_base & 3))
        return fail(SE_EINVAL, "env_id_base must be a multiple of 4 (envs 4k..4k+3 share draw blocks)");
    if (H < 1 || W < 1 || H > SE_MAX_SIDE || W > SE_MAX_SIDE)
        return fail(SE_EINVAL, "map sides must be in [1, 256]");
    if (!water) return fail(SE_EINVAL, "null water map");
    if (P > 0 && (!port_x || !port_y || !port_fuel || !port_cargo))
        return fail(SE_EINVAL, "null port arrays");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(SE_EINVAL, "bad device ordinal");
    DeviceGuard g(device);
    se_env* env = new se_env();
    env->device = device;
    env->n = n;
    env->env_base = env_id_base;
    env->seed = seed;
    env->flags = flags;
    env->dims.H = H;
    env->dims.W = W;
    env->water.assign(water, water + (size_t)H * W);
    for (auto& v : env->water) v = v ? 1 : 0;
    int rc = upload_world(env, P, port_x, port_y, port_fuel, port_cargo);
    if (rc) {
        se_destroy(env);
        return rc;
    }
    {
        // workgroup b owns iters * 256 consecutive groups of 4 envs
        const int64_t groups = (n + kEnvsPerThread - 1) / kEnvsPerThread;
        const int64_t cap = step_block_cap();
        env->iters = groups > 0 ? (groups + cap * kStepBlock - 1) / (cap * kStepBlock) : 1;
        env->grid = (int)(groups > 0 ? (groups + env->iters * kStepBlock - 1) / (env->iters * kStepBlock) : 1);
        env->seg = 64 * kEnvsPerThread;  // one done-list segment per (iteration, wave)
        env->nseg = (int64_t)env->grid * env->iters * (kStepBlock / 64);
        env->nslab = (int64_t)env->grid * (kStepBlock / 64);  // stats: one entry per wave
        env->done_pad = done_pad_records(env);
        env->nt_loads = step_nt_loads(env);
        env->seq_fuse = seq_fuse();
        env->seq_max_steps = seq_max_steps();
        env->seq_gate_pool = seq_gate_pool();
        env->seq_ring = seq_ring();
        env->seq_screen = seq_screen();
        env->mask_tiled = mask_tiled();
    }
    hipError_t e = hipMalloc(&env->d_slab, (size_t)env->nslab * 4 * sizeof(double));
    if (e == hipSuccess) e = hipMemset(env->d_slab, 0, (size_t)env->nslab * 4 * sizeof(double));
    if (e != hipSuccess) {
        se_destroy(env);
        return fail(SE_EHIP, std::string("se_create allocation: ") + hipGetErrorString(e));
    }
    *out = env;
    return SE_OK;
}

int se_set_ports(se_env* env, int32_t P, const int32_t* port_x, const int32_t* port_y,
                 const int32_t* port_fuel, const int32_t* port_cargo) {
    if (!env) return fail(SE_EINVAL, "null env");
    if (P > 0 && (!port_x || !port_y || !port_fuel || !port_cargo))
        return fail(SE_EINVAL, "null port arrays");
    DeviceGuard g(env->device);
    HIP_TRY(hipDeviceSynchronize());  // the old image may still be read by queued work
    return upload_world(env, P, port_x, port_y, port_fuel, port_cargo);
}

int se_bind(se_env* env, const se_state* st) {
    if (!env || !st) return fail(SE_EINVAL, "null argument");
    const void* req[] = {st->x, st->y, st->fuel, st->cargo, st->origin, st->dest,
                         st->reward, st->done, st->err};
    for (const void* p : req) {
        if (!p && env->n > 0) return fail(SE_EINVAL, "null state buffer");
        if (!aligned16(p)) return fail(SE_EINVAL, "state buffers must be 16-byte aligned");
    }
    if (env->flags & SE_FLAG_AUTO_RESET) {
        if ((env->n > 0 && (!st->ep_return || !st->ep_start)) || !st->done_recs || !st->done_count)
            return fail(SE_EINVAL, "auto-reset needs ep_return, ep_start, done_recs and done_count");
        if (!aligned16(st->ep_return) || !aligned16(st->ep_start) || !aligned16(st->done_recs))
            return fail(SE_EINVAL, "state buffers must be 16-byte aligned");
        DeviceGuard g(env->device);
        HIP_TRY(hipMemset(st->done_count, 0, 2 * (size_t)env->nseg * sizeof(int32_t)));
    }
    env->st = *st;
    env->bound = true;
    return SE_OK;
}

int se_reset(se_env* env, const uint8_t* mask, void* stream) {
    int rc = check_ready(env);
    if (rc) return rc;
    if (env->dims.P < 2) return fail(SE_EINVAL, "reset needs at least two ports");
    rc = launch_reset(env, mask, nullptr, nullptr, stream);
    if (rc) return rc;
    env->epoch += 1;
    return SE_OK;
}

int se_reset_to(se_env* env, const uint8_t* mask, const int32_t* origin, const int32_t* dest,
                void* stream) {
    int rc = check_ready(env);
    if (rc) return rc;
    if (env->n > 0 && (!origin || !dest)) return fail(SE_EINVAL, "null origin/dest");
    return launch_reset(env, mask, origin, dest, stream);  // the epoch stays: no draw was made
}

int se_step(se_env* env, const int32_t* actions, void* stream) {
    return launch_step(env, false, false, actions, nullptr, nullptr, nullptr, stream);
}

int se_step_seq_mark(se_env* env, const int32_t* actions, int64_t ld, int32_t steps, void* stream,
                     void* event, int32_t mark_after) {
    int rc = check_ready(env);
    if (rc) return rc;
    if (steps < 0) return fail(SE_EINVAL, "negative step count");
    if (steps > 1 && (ld < env->n || (ld & 3))) return fail(SE_EINVAL, "row stride must be >= n and a multiple of 4");
    if (event && (mark_after < 0 || mark_after > steps)) return fail(SE_EINVAL, "mark_after must be in [0, steps]");
    // without auto-reset nothing reads the state between two steps of the run: fused launches
    // (step_seq_kernel), split where the event goes and at seq_max_steps. Auto-reset keeps a
    // launch per step (its done lists and statistics are per step).
    // A world image that fills the 64 KiB a launch can ask for leaves no room for the fused
    // kernel's stock table: such an env steps per launch, as step_kernel still fits.
    const bool fused = env->seq_fuse && env->n > 0 && !(env->flags & SE_FLAG_AUTO_RESET) &&
                       lds_bytes(env) + kStockByCodeBytes <= kLdsDefault;
    for (int32_t k = 0; k <= steps;) {
        if (event && k == mark_after) {
            DeviceGuard g(env->device);
            HIP_TRY(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
        }
        if (k == steps) break;
        if (fused) {
            const int32_t end = event && k < mark_after ? mark_after : steps;
            const int32_t run = std::min(end - k, env->seq_max_steps);
            rc = launch_step_seq(env, actions + (int64_t)k * ld, ld, run, stream);
            k += run;
        } else {
            rc = launch_step(env, false, false, actions + (int64_t)k * ld, nullptr, nullptr, nullptr, stream, nullptr, true);
            k += 1;
        }
        if (rc) return rc;
    }
    return SE_OK;
}

int se_step_seq(se_env* env, const int32_t* actions, int64_t ld, int32_t steps, void* stream) {
    return se_step_seq_mark(env, actions, ld, steps, stream, nullptr, 0);
}

int se_step_typed(se_env* env, const int32_t* type, const int32_t* a, const int32_t* b,
                  void* stream) {
    return launch_step(env, true, false, type, a, b, nullptr, stream);
}

int se_step_replay(se_env* env, const int32_t* type, const int32_t* a, const int32_t* b,
                   se_tape* tape, void* stream) {
    return launch_step(env, true, true, type, a, b, tape, stream);
}

int se_step_agent_replay(se_env* env, const int32_t* actions, se_tape* tape, void* stream) {
    return launch_step(env, false, true, actions, nullptr, nullptr, tape, stream);
}

int se_observe(se_env* env, float* obs, int64_t ld, void* stream) {
    int rc = check_ready(env);
    if (rc) return rc;
    if ((env->n > 0 && !obs) || ld < 6 + 4 * (int64_t)env->dims.P) return fail(SE_EINVAL, "bad obs buffer / ld");
    DeviceGuard g(env->device);
    ObsArgs A{env->d_world, env->dims, env->n, ld, env->st, obs};
    const int64_t W = 6 + 4 * (int64_t)env->dims.P;
    const int64_t total = env->n * W;
    if (total == 0) return SE_OK;
    if (ld == W && aligned16(obs) && W <= 1022) {  // dense rows: the tiled kernel
        const uint32_t magic = (uint32_t)((((uint64_t)1 << 32) + (uint64_t)W - 1) / (uint64_t)W);
        const size_t lds = (size_t)(kTileRows * 6 + 4 * env->dims.P) * sizeof(float);
        observe_tiled_kernel<<<grid_for(env->n), kBlock, lds, (hipStream_t)stream>>>(A, magic);
    } else {
        observe_kernel<<<grid_for(total), kBlock, lds_bytes(env), (hipStream_t)stream>>>(A);
    }
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

int se_valid_mask(se_env* env, uint8_t* bits, void* stream) {
    int rc = check_ready(env);
    if (rc) return rc;
    if (env->n > 0 && !bits) return fail(SE_EINVAL, "null bits");
    DeviceGuard g(env->device);
    const int32_t stride = (4 + env->dims.P + 250 + 7) / 8;
    MaskArgs A{env->d_world, env->dims, env->n, stride, env->st, bits};
    const int64_t total = env->n * stride;
    if (total == 0) return SE_OK;
    const hipStream_t s = (hipStream_t)stream;
    const int tb = mask_tb(stride);
    if (aligned16(bits) && env->dims.P <= 64 && env->mask_ntmpl <= kMaskTmplMax && !env->mask_tiled) {
        // the row templates, rebuilt when the world image changed
        const size_t need = (size_t)kMaskHdr + (size_t)env->mask_ntmpl * tb;
        if (need > env->mask_tmpl_cap) env->mask_tmpl_version = 0;  // a new block holds no templates
        rc = device_reserve(env->d_mask_tmpl, env->mask_tmpl_cap, need);
        if (rc) return rc;
        if (env->mask_tmpl_version != env->world_version) {
            mask_tmpl_kernel<<<1, kBlock, 0, s>>>(env->d_world, env->dims, stride, env->d_mask_tmpl);
            HIP_TRY(hipGetLastError());
            env->mask_tmpl_version = env->world_version;
        }
        const uint32_t magic = (uint32_t)((((uint64_t)1 << 32) + (uint64_t)stride - 1) / (uint64_t)stride);
        const size_t lds = (size_t)env->mask_ntmpl * tb;
        valid_mask_tmpl_kernel<<<grid_for(env->n, lds > 4096 ? 1024 : kMaxBlocks), kBlock, lds, s>>>(
            A, env->d_mask_tmpl, env->mask_ntmpl, magic);
    } else if (aligned16(bits)) {  // the tiled kernel (rows are always dense here)
        const size_t lds = ((size_t)kTileRows * stride + 15) & ~(size_t)15;
        valid_mask_tiled_kernel<<<grid_for(env->n), kBlock, lds, s>>>(A);
    } else {
        valid_mask_kernel<<<grid_for(total), kBlock, lds_bytes(env), (hipStream_t)stream>>>(A);
    }
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

int se_gen_actions(se_env* env, int32_t* actions, uint32_t t, void* stream) {
    if (!env || (!actions && env->n > 0)) return fail(SE_EINVAL, "null argument");
    if (!aligned16(actions)) return fail(SE_EINVAL, "actions must be 16-byte aligned");
    if (env->dims.P < 1) return fail(SE_EINVAL, "the synthetic agent needs ports");
    DeviceGuard g(env->device);
    if (env->n > 0) {
        gen_actions_kernel<<<grid_for(env->n), kBlock, 0, (hipStream_t)stream>>>(
            env->n, env->env_base, env->seed, t, env->dims.P, actions);
        HIP_TRY(hipGetLastError());
    }
    return SE_OK;
}

int se_sample_actions(se_env* env, int32_t* type, int32_t* a, int32_t* b, uint32_t t, void* stream) {
    int rc = check_ready(env);
    if (rc) return rc;
    if (env->n == 0) return SE_OK;
    if (!type || !a || !b) return fail(SE_EINVAL, "null output pointer");
    DeviceGuard g(env->device);
    const SampleArgs A{env_args(env), t, type, a, b};
    sample_kernel<<<grid_for(env->n), kBlock, 0, (hipStream_t)stream>>>(A);
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

int se_rollout(se_env* env, const int32_t* src, int64_t m, int32_t max_steps, int32_t max_attempts,
               int64_t rollout_base, double* ret, int32_t* steps, int32_t* status, void* stream) {
    int rc = check_ready(env);
    if (rc) return rc;
    if (m < 0 || max_steps < 0 || max_attempts < 0 || rollout_base < 0)
        return fail(SE_EINVAL, "m, max_steps, max_attempts and rollout_base must be >= 0");
    if (m > 0 && (!src || !ret || !steps || !status)) return fail(SE_EINVAL, "null rollout buffer");
    if (m == 0) return SE_OK;
    DeviceGuard g(env->device);
    const RolloutArgs A{env_args(env), m, rollout_base, max_steps, max_attempts, src, ret, steps, status};
    rollout_kernel<<<grid_for(m), kBlock, lds_bytes(env), (hipStream_t)stream>>>(A);
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

int se_rollout_plan(se_env* env, const int32_t* src, int64_t m, const int32_t* type, const int32_t* a,
                    const int32_t* b, int64_t ld, int32_t steps, const int32_t* len, const int64_t* ids,
                    int64_t rollout_base, double* ret, int32_t* counted, int32_t* status,
                    const se_plan_out* out, void* stream) {
    // the arguments first: misuse is reported whatever the env's state
    if (m < 0 || steps < 0 || rollout_base < 0)
        return fail(SE_EINVAL, "m, steps and rollout_base must be >= 0");
    if ((a == nullptr) != (b == nullptr))
        return fail(SE_EINVAL, "a and b go together: both for typed actions, neither for agent indices");
    if (ld < m) return fail(SE_EINVAL, "row stride must be >= m");
    if (m > 0 && (!src || !ret || !counted || !status || (steps > 0 && !type)))
        return fail(SE_EINVAL, "null plan buffer");
    if (!aligned16(type) || !aligned16(a) || !aligned16(b) || (steps > 1 && (ld & 3)))
        return fail(SE_EINVAL, "plan rows must be 16-byte aligned (row stride a multiple of 4)");
    int rc = check_ready(env);
    if (rc) return rc;
    if (m == 0) return SE_OK;
    DeviceGuard g(env->device);
    const bool agent = a == nullptr;
    size_t lds;
    rc = agent ? world_lds<plan_kernel<true>>(env, lds) : world_lds<plan_kernel<false>>(env, lds);
    if (rc) return rc;
    PlanArgs A{};
    static_cast<EpisodeArgs&>(A) = {env_args(env), m, rollout_base, src, ids, ret, counted, status};
    A.ld = ld;
    A.steps = steps;
    A.type = type;
    A.a = a;
    A.b = b;
    A.len = len;
    if (out) A.out = *out;
    const auto kernel = agent ? plan_kernel<true> : plan_kernel<false>;
    kernel<<<grid_for(m), kBlock, lds, (hipStream_t)stream>>>(A);
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

int se_episode_stats(se_env* env, double* out, void* stream) {
    if (!env || !out) return fail(SE_EINVAL, "null argument");
    DeviceGuard g(env->device);
    stats_kernel<<<1, kStatsBlock, 0, (hipStream_t)stream>>>(env->d_slab, (int)env->nslab, out);
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

int se_clear_stats(se_env* env, void* stream) {
    if (!env) return fail(SE_EINVAL, "null env");
    DeviceGuard g(env->device);
    HIP_TRY(hipMemsetAsync(env->d_slab, 0, (size_t)env->nslab * 4 * sizeof(double),
                           (hipStream_t)stream));
    return SE_OK;
}

int se_done_layout(se_env* env, int64_t* seg_stride, int32_t* segments) {
    if (!env) return fail(SE_EINVAL, "null env");
    if (seg_stride) *seg_stride = env->seg;
    if (segments) *segments = (int32_t)env->nseg;
    return SE_OK;
}

int se_done_list(se_env* env, int64_t* rec_offset, int64_t* count_offset) {
    if (!env || !rec_offset || !count_offset) return fail(SE_EINVAL, "null argument");
    if (!(env->flags & SE_FLAG_AUTO_RESET)) return fail(SE_ESTATE, "no done list without auto-reset");
    if (env->step_t == 0) return fail(SE_ESTATE, "no step has run");
    const int64_t par = (int64_t)((env->step_t - 1) & 1u);
    *rec_offset = par * (int64_t)env->nseg * env->seg;
    *count_offset = par * (int64_t)env->nseg;
    return SE_OK;
}

int se_done_compact(se_env* env, se_done_rec* out, int32_t* out_count, void* stream) {
    int64_t ro = 0, co = 0;
    int rc = se_done_list(env, &ro, &co);
    if (rc) return rc;
    if (!out || !out_count) return fail(SE_EINVAL, "null output");
    DeviceGuard g(env->device);
    if (!env->d_offsets) HIP_TRY(hipMalloc(&env->d_offsets, (size_t)env->nseg * sizeof(int32_t)));
    const hipStream_t s = (hipStream_t)stream;
    done_scan_kernel<<<1, 1024, 0, s>>>(env->st.done_count + co, env->nseg, env->d_offsets, out_count);
    const int64_t blocks = (env->nseg + kBlock / 64 - 1) / (kBlock / 64);
    done_copy_kernel<<<(int)blocks, kBlock, 0, s>>>(env->st.done_recs + ro, env->st.done_count + co,
                                                    env->d_offsets, env->nseg, env->seg, out);
    HIP_TRY(hipGetLastError());
    return SE_OK;
}

int se_get_counters(se_env* env, uint64_t* step, uint64_t* epoch) {
    if (!env) return fail(SE_EINVAL, "null env");
    if (step) *step = env->step_t;
    if (epoch) *epoch = env->epoch;
    return SE_OK;
}

int se_set_counters(se_env* env, uint64_t step, uint64_t epoch) {
    if (!env) return fail(SE_EINVAL, "null env");
    DeviceGuard g(env->device);
    HIP_TRY(hipDeviceSynchronize());
    if (env->bound && env->st.done_count)
        HIP_TRY(hipMemset(env->st.done_count, 0, 2 * (size_t)env->nseg * sizeof(int32_t)));
    env->step_t = step;
    env->epoch = epoch;
    return SE_OK;
}

int se_destroy(se_env* env) {
    if (!env) return SE_OK;
    DeviceGuard g(env->device);
    (void)device_free({env->d_world, env->d_slab, env->d_offsets, env->d_mask_tmpl});
    delete env;
    return SE_OK;
}

// ---------------------------------------------------------------- host-resident envs
int se_host_create(se_host** out, int32_t H, int32_t W, const uint8_t* water, int32_t P,
                   const int32_t* port_x, const int32_t* port_y, const int32_t* port_fuel,
                   const int32_t* port_cargo) {
    if (!out) return fail(SE_EINVAL, "null out");
    *out = nullptr;
    if (H < 1 || W < 1 || H > SE_MAX_SIDE || W > SE_MAX_SIDE)
        return fail(SE_EINVAL, "map sides must be in [1, 256]");
    if (!water) return fail(SE_EINVAL, "null water map");
    if (P > 0 && (!port_x || !port_y || !port_fuel || !port_cargo)) return fail(SE_EINVAL, "null port arrays");
    se_host* h = new se_host();
    h->dims.H = H;
    h->dims.W = W;
    h->water.assign(water, water + (size_t)H * W);
    for (auto& v : h->water) v = v ? 1 : 0;
    const int rc = build_world_image(H, W, h->water, P, port_x, port_y, port_fuel, port_cargo, h->dims, h->img);
    if (rc) {
        delete h;
        return rc;
    }
    *out = h;
    return SE_OK;
}

int se_host_set_ports(se_host* h, int32_t P, const int32_t* port_x, const int32_t* port_y,
                      const int32_t* port_fuel, const int32_t* port_cargo) {
    if (!h) return fail(SE_EINVAL, "null host world");
    if (P > 0 && (!port_x || !port_y || !port_fuel || !port_cargo)) return fail(SE_EINVAL, "null port arrays");
    return build_world_image(h->dims.H, h->dims.W, h->water, P, port_x, port_y, port_fuel, port_cargo, h->dims,
                             h->img);
}

int se_host_step_replay(se_host* h, int64_t n, const se_state* st, const int32_t* type, const int32_t* a,
                        const int32_t* b, se_tape* tape) {
    if (!h || !st || n < 0) return fail(SE_EINVAL, "null argument or n < 0");
    if (n == 0) return SE_OK;
    if (!type || !a || !b || !tape || !st->x || !st->y || !st->fuel || !st->cargo || !st->origin || !st->dest ||
        !st->reward || !st->done || !st->err)
        return fail(SE_EINVAL, "null state, action or tape buffer");
    const LdsWorld w = world_view(h->dims, h->img.data());
    for (int64_t i = 0; i < n; ++i) {
        Ship s = load_ship(*st, i);
        Pending p;
        se_tape* tp = tape + i;
        tp->used = (int32_t)replay_env(w, s, p, SE_ERR_OK, type[i], a[i], b[i], tp->u_fuel, tp->u_gate, tp);
        store_ship(*st, i, s);
        st->reward[i] = (float)p.r;  // one rounding of the reference's f64 reward
        st->done[i] = (uint8_t)p.dead;
        st->err[i] = (int8_t)p.e;
        if (st->reward64) st->reward64[i] = p.r;
    }
    return SE_OK;
}

int se_host_reset_to(se_host* h, int64_t n, const se_state* st, const uint8_t* mask, const int32_t* origin,
                     const int32_t* dest) {
    if (!h || !st || n < 0 || (n > 0 && (!origin || !dest))) return fail(SE_EINVAL, "null argument or n < 0");
    const LdsWorld w = world_view(h->dims, h->img.data());
    for (int64_t i = 0; i < n; ++i)
        if ((!mask || mask[i]) && (origin[i] < 0 || origin[i] >= w.P || dest[i] < 0 || dest[i] >= w.P))
            return fail(SE_EINVAL, "origin / dest must name ports");
    for (int64_t i = 0; i < n; ++i) {  // reset_kernel's explicit form (reset() :227-243)
        if (mask && !mask[i]) continue;
        st->x[i] = (uint8_t)w.px(origin[i]);
        st->y[i] = (uint8_t)w.py(origin[i]);
        st->fuel[i] = kFuelInit;
        st->cargo[i] = 0;
        st->origin[i] = (uint8_t)origin[i];
        st->dest[i] = (uint8_t)dest[i];
        if (st->ep_return) st->ep_return[i] = 0.0f;
        if (st->ep_start) st->ep_start[i] = 0;  // a host world has no step counter
        st->done[i] = 0;
        st->err[i] = 0;
        st->reward[i] = 0.0f;
    }
    return SE_OK;
}

int se_host_destroy(se_host* h) {
    delete h;
    return SE_OK;
}

}  // extern "C"

// the fused DQN policy step (same translation unit: world image, env handle, Philox)
#include "qpolicy.h"
#include "qnet_rollout.h"  // after qpolicy.h: plays its packed image on episode.h's scaffold
#include "nav.h"  // before mcts.h: se_mcts_choose_nav plays the navigator
#include "mcts.h"
#include "sarsa.h"
#include "sarsa_rollout.h"  // after sarsa.h: plays its tables through sarsa_choose
#include "replay.h"
#include "qtrain.h"
#include "server.h"
