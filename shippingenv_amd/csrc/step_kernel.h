#pragma once
// step_kernel.h — the step kernels around the group steps: the fixed-order wave
// sums (wave_sum*), slab_add, the done list's wave_compact, step_kernel, and the
// partial last group's step_tail_envs / step_tail_kernel.
//
// A fragment of shipenv.hip's translation unit, included inside its anonymous
// namespace where this text stood: not a stand-alone header.
// Uses world.h (stage_issue / stage_finish, world_view), env_core.h (count_below),
// step_io.h (StepArgs, Group, At), step_group.h (step_group, BlockStats, Finished)
// and step_agent.h (step_group_agent, early_draws, the record helpers).

// Sum over the wave's 64 lanes in a fixed tree, so the result does not depend on
// timing: within each row of 16 lanes, DPP exchanges with lane^1, lane^2, the
// mirrored lane of the half row and of the row (every lane then holds its row's
// sum; each exchange pairs two lanes symmetrically and f64 addition commutes, so
// both hold identical bits), then the four row sums as (r0 + r1) + (r2 + r3).
// No LDS round trips (a shuffle butterfly cost 36 ds_bpermute and 6 dependent
// waits at the end of every wave).
template <int kCtrl>
__device__ __forceinline__ double dpp_f64(double v) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)b, kCtrl, 0xf, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(b >> 32), kCtrl, 0xf, 0xf, false);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
constexpr int kDppXor1 = 0xb1;        // quad_perm [1, 0, 3, 2]
constexpr int kDppXor2 = 0x4e;        // quad_perm [2, 3, 0, 1]
constexpr int kDppHalfMirror = 0x141; // row_half_mirror
constexpr int kDppMirror = 0x140;     // row_mirror
__device__ __forceinline__ double wave_sum(double v) {
    v += dpp_f64<kDppXor1>(v);
    v += dpp_f64<kDppXor2>(v);
    v += dpp_f64<kDppHalfMirror>(v);
    v += dpp_f64<kDppMirror>(v);
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    double r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, 16 * k);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), 16 * k);
        r[k] = __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
    }
    return (r[0] + r[1]) + (r[2] + r[3]);
}
__device__ __forceinline__ int wave_sum_int(int v) {
    v += __builtin_amdgcn_mov_dpp(v, kDppXor1, 0xf, 0xf, false);
    v += __builtin_amdgcn_mov_dpp(v, kDppXor2, 0xf, 0xf, false);
    v += __builtin_amdgcn_mov_dpp(v, kDppHalfMirror, 0xf, 0xf, false);
    v += __builtin_amdgcn_mov_dpp(v, kDppMirror, 0xf, 0xf, false);
    return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) +
           (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}

// Statistics slab update: lanes 0-2 of each wave load the
// wave's entry at the kernel's start and store old + sum at its end (plain loads and stores;
// the entry is this wave's alone during a launch). At N = 2^24 the three no-return f64
// atomics per wave (memory-side 64-B requests) cost config 4 ~16 us of ~190
// (a timing-only ablation, profiles/r04/c4split.jsonl).
// slab[i] += v without reading it back into the wave: the add runs in L2 and the
// wave does not wait for it. Only this wave's lane 0 adds to its own entry during
// a launch (step_tail_kernel adds in a later launch), so the order of additions is
// fixed and the sums are deterministic.
__device__ __forceinline__ void slab_add(double* p, double v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Done-list compaction of one iteration (auto-reset): no atomics, no LDS and no
// barrier. A wave-exclusive prefix of the per-lane counts (0..4) comes from three
// ballot bit-planes; the records go to this wave's own segment of the list in env
// order (deterministic). An earlier version ranked the waves of a workgroup through
// LDS behind two barriers: 1.4 us of a 15.4 us config-4 step.
__device__ __forceinline__ void wave_compact(const StepArgs& A, const Finished& F, int64_t base,
                                             int64_t segment) {
    const int nd = __popc(F.mask);
    const uint64_t b0 = __ballot(nd & 1), b1 = __ballot(nd & 2), b2 = __ballot(nd & 4);
    if (nd) {
        int64_t slot = segment * A.seg + (int32_t)(count_below(b0) + 2 * count_below(b1) + 4 * count_below(b2));
        const int32_t t = (int32_t)A.t;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((F.mask >> j) & 1u) A.done_recs[slot++] = se_done_rec{(int32_t)(base + j), F.ret[j], F.len[j], t};
    }
    const int32_t total = (int32_t)(__popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2));
    if (A.done_pad > 1) {  // launch-uniform (done_pad_records)
        // the wave's records padded to whole lines with filler records (env -1) past the
        // count: a line of the list written in part by one wave leaves L2 as a partial-line
        // write, and at N = 2^24 the ~1 record per wave cost config 4 ~11 us of ~192
        // (a timing-only ablation, profiles/r04/ab_c4parts.jsonl). A segment holds 256
        // records, a multiple of the pad, so the filler stays inside it.
        const int32_t pad = (-total) & (A.done_pad - 1), l = (int32_t)(threadIdx.x & 63);
        if (total != 0 && l < pad)
            A.done_recs[segment * A.seg + total + l] = se_done_rec{-1, 0.0f, 0, (int32_t)A.t};
    }
    if ((threadIdx.x & 63) == 0) A.done_count[segment] = total;
}

// Workgroup b owns the contiguous groups [b*iters*256, (b+1)*iters*256) (a group is
// 4 consecutive envs, one lane per group per iteration). In iteration k, wave w
// steps the 64 groups from b*iters*256 + k*256 + w*64: its done-list segment
// (segment = global group / 64) covers them in env order, so the concatenated
// segments are globally sorted. Every field of a group is one 4- or
// 16-byte lane access. The partial last group (n % 4 envs) is left to
// step_tail_kernel, so this loop carries no guarded scalar path. The world image's
// loads, then the first group's, are all in flight before the LDS writes; each
// iteration loads the next group after storing the current one.
// kSeq: the same code, instantiated apart for se_step_seq's launches (the agent path without
// auto-reset), so a kernel trace lists them under a name of their own: bench.py's headline leg
// issues its timed steps that way, and its trace row then holds exactly those launches.
template <bool kTyped, bool kReplay, bool kAuto, bool kNt = false, bool kRec = false, bool kSeq = false>
__global__ __launch_bounds__(kStepBlock) __attribute__((amdgpu_waves_per_eu(4))) void step_kernel(StepArgs A) {
    static_assert(!kRec || (kAuto && !kTyped && !kReplay), "se_step_record: agent actions, auto-reset");
    extern __shared__ uint32_t lds[];
    const int64_t full = A.n >> 2;
    const int64_t first = (int64_t)blockIdx.x * A.iters * kStepBlock;  // block-uniform first group

    TRACE_STAMP(0);
    const Staged st = stage_issue(A.world);
    // the image's loads first: the staging writes then wait for them alone
    __builtin_amdgcn_sched_barrier(0);
    // first group: an unconditional load (lanes past the end re-read the last full
    // group; the host launches this kernel only when there is one), so the staging
    // writes below wait for exactly the image's loads
    Group<kTyped, kAuto, kNt> G;
    {
        const int64_t last = full - 1 - first;  // block-uniform
        const uint32_t lane = last < (int64_t)threadIdx.x ? (uint32_t)(last < 0 ? 0 : last) : threadIdx.x;
        G.template load<true>(A, At<true>{last < 0 ? full - 1 : first, 0, A.n}, lane);
    }
    __builtin_amdgcn_sched_barrier(0);
    // auto-reset: this wave's statistics so far ({sum ret, episodes, sum len} on lanes 0-2),
    // loaded now so the end of the wave adds to them without waiting
    // (kRec keeps the atomics: two more registers there spilled)
    constexpr bool kSlabRmw = kAuto && !kRec;
    [[maybe_unused]] double slab_prev = 0.0;
    if constexpr (kSlabRmw) {
        const uint32_t l = threadIdx.x & 63;
        const double* sl = late_args().slab + 4 * (blockIdx.x * (kStepBlock / 64) + (threadIdx.x >> 6));
        slab_prev = sl[l < 3 ? l : 0];
    }
    // agent-index actions: the production step, or its replay-tape form (parity)
    constexpr bool kAgent = !kTyped;
    constexpr bool kDraws = kAgent && !kReplay;
    Draws D{};
    if constexpr (kDraws) {
        D = early_draws<spec_loss<kAuto>()>(A, (first + threadIdx.x) * 4);
        // keep the draws ahead of the staging wait: they overlap the loads in flight
        asm volatile("" : "+v"(D.fuel.v[0]), "+v"(D.gate.v[0]), "+v"(D.loss0.v[0]), "+v"(D.arrive.v[0]));
    }
    const LdsWorld w = stage_finish(A.world, A.dims, lds, st);
    TRACE_STAMP(1);

    BlockStats bs;
    uint32_t cuts = 0;  // kRec: bit 4k + j = env j of this thread's group k restarts
    for (int64_t k = 0; k < A.iters; ++k) {
        const int64_t g0 = first + k * kStepBlock, g = g0 + threadIdx.x;
        Finished F;
        const bool more = k + 1 < A.iters && g + kStepBlock < full;
        if (g < full) {
            if constexpr (kAgent) {
                if constexpr (kDraws) {
                    if (k > 0) D = early_draws<spec_loss<kAuto>()>(A, g * 4);
                }
                step_group_agent<kAuto, true, kNt, kRec, kReplay>(A, w, G, At<true>{g0, g * 4, A.n}, bs, F, D);
                if constexpr (kRec) cuts |= F.cut << (4 * k);
            } else
                step_group<kTyped, kReplay, kAuto, true, kNt>(A, w, G, At<true>{g0, g * 4, A.n}, bs, F);
            if (k == 0) TRACE_STAMP(2);
            if (more) G.template load<true>(A, At<true>{g0 + kStepBlock, 0, A.n});
        }
        // done-list segment of this (iteration, wave): 64 groups, in env order
        if constexpr (kAuto) wave_compact(late_args(), F, g * 4, __builtin_amdgcn_readfirstlane((int32_t)(g >> 6)));
    }

#if SHIPENV_TRACE
    __builtin_amdgcn_s_waitcnt(0);  // stores acknowledged
    TRACE_STAMP(3);
#endif
    if constexpr (kRec) {  // the ring's stored count, read by the sampler (replay_end4_kernel)
        if (blockIdx.x == 0 && threadIdx.x == 0) *late_args().rec.d_size = late_args().rec.new_size;
        if (cuts) record_restart(late_args(), w, cuts);
    }
    if (kAuto) {
        // per-wave statistics: a fixed-order tree (wave_sum), added to this wave's own
        // slab entry. With episodes ending about once per 240 steps, most waves have one
        // lane with a finished episode or none: then that lane's values are the sums
        // (every other lane adds +0.0, which the tree's f64 adds leave exact), read
        // with three readlanes instead of three trees.
        const uint64_t ended = __ballot(bs.eps != 0);
        if (ended == 0) return;
        double ret, len;
        int eps;
        if ((ended & (ended - 1)) == 0) {
            const int src = __builtin_ctzll(ended);
            const uint64_t rb = __builtin_bit_cast(uint64_t, bs.ret);
            ret = __builtin_bit_cast(double, (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(rb >> 32), src) << 32 |
                                                 (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)rb, src));
            len = (double)__builtin_amdgcn_readlane(bs.len, src);
            eps = __builtin_amdgcn_readlane(bs.eps, src);
        } else {
            ret = wave_sum(bs.ret);
            len = wave_sum((double)bs.len);
            eps = wave_sum_int(bs.eps);
        }
        if constexpr (!kSlabRmw) {
            if (eps != 0 && (threadIdx.x & 63) == 0) {
                double* sl = late_args().slab + 4 * (blockIdx.x * (kStepBlock / 64) + (threadIdx.x >> 6));
                slab_add(sl + 0, ret);
                slab_add(sl + 1, (double)eps);
                slab_add(sl + 2, len);
            }
        } else if (eps != 0 && (threadIdx.x & 63) < 3) {
            // the same additions in the same order as a read-modify-write from registers:
            // lanes 0-2 hold the entry's old values (loaded at the kernel's start), and no
            // other wave touches this entry during the launch
            const uint32_t l = threadIdx.x & 63;
            double* sl = late_args().slab + 4 * (blockIdx.x * (kStepBlock / 64) + (threadIdx.x >> 6));
            sl[l] = slab_prev + (l == 0 ? ret : l == 1 ? (double)eps : len);
        }
    }
}

// The partial last group (n % 4 envs), launched after step_kernel on the same
// stream when n % 4 != 0: one thread steps it with guarded scalar accesses. Its
// envs come last in env order, so auto-reset appends their records to the done
// segment of group n/4 after step_kernel's and adds their statistics to the slab
// entry of the wave that owns that group (env order and a fixed summation order,
// as in the main kernel).
template <bool kTyped, bool kReplay, bool kAuto>
__device__ __forceinline__ void step_tail_envs(const StepArgs& A, const LdsWorld& w) {
    // at most 3 envs: step_tail_kernel reads the world in place (L2), not staged, so the step
    // starts without the staging round trips (the N = 1 launch path is this kernel alone)
    const int64_t g = A.n >> 2;
    const At<false> at{0, g * 4, A.n};
    Group<kTyped, kAuto> G;
    G.template load<false>(A, at);
    BlockStats bs;
    Finished F;
    if constexpr (!kTyped && !kReplay)
        step_group_agent<kAuto, false, false>(A, w, G, at, bs, F, early_draws<spec_loss<kAuto>()>(A, at.base));
    else if constexpr (!kTyped && kReplay)
        step_group_agent<kAuto, false, false, false, true>(A, w, G, at, bs, F, Draws{});
    else
        step_group<kTyped, kReplay, kAuto, false>(A, w, G, at, bs, F);
    if constexpr (kAuto) {
        const int64_t b = g >> 6;  // the (iteration, wave) segment that owns group g
        int32_t c = (g & 63) == 0 ? 0 : A.done_count[b];  // a fresh segment: step_kernel wrote none
        for (int j = 0; j < 4; ++j)
            if ((F.mask >> j) & 1u)
                A.done_recs[b * A.seg + c++] = se_done_rec{(int32_t)(at.base + j), F.ret[j], F.len[j], (int32_t)A.t};
        A.done_count[b] = c;
        // fewer than 4 envs: step_kernel did not run, so the other waves' segments of the one
        // workgroup (se_done_layout still counts them) get their count of this step here
        if (A.n < kEnvsPerThread)
            for (int s = 1; s < kStepBlock / 64; ++s) A.done_count[s] = 0;
        if (bs.eps != 0) {
            // the slab entry of the wave that owns group g
            const int64_t bl = g / (A.iters * kStepBlock), wv = (g % kStepBlock) >> 6;
            double* sl = A.slab + 4 * (bl * (kStepBlock / 64) + wv);
            sl[0] += bs.ret;
            sl[1] += (double)bs.eps;
            sl[2] += (double)bs.len;
        }
    }
}

template <bool kTyped, bool kReplay, bool kAuto>
__global__ __launch_bounds__(64) void step_tail_kernel(StepArgs A) {
    if (threadIdx.x != 0) return;
    step_tail_envs<kTyped, kReplay, kAuto>(A, world_view(A.dims, A.world));
}
