#pragma once
// step_io.h — what a step kernel is handed and how it moves a group of 4 envs:
// the trace stamps of the diagnostic build, StepRecord (the training loop's record
// contract, also replay.h's), StepArgs, late_args, the streaming ld* / st* accesses,
// At, Group, and the stamp and store helpers.
//
// A fragment of shipenv.hip's translation unit, included inside its anonymous
// namespace where this text stood: not a stand-alone header.
// Uses world.h (WorldDims) and include/shipenv.h (se_state, se_tape).

// ------------------------------------------------------------------ step kernel
#if SHIPENV_TRACE
// [step parity][wave][8] s_memrealtime stamps (100 MHz): start, staged, stepped, end
constexpr int kTraceWaves = 1 << 16;
__device__ uint64_t g_trace[kTraceWaves * 8];
#define TRACE_STAMP(k)                                                                        \
    do {                                                                                      \
        const uint64_t t_ = __builtin_amdgcn_s_memrealtime();                                 \
        const uint32_t w_ = blockIdx.x * (kStepBlock / 64) + (threadIdx.x >> 6);                  \
        if ((threadIdx.x & 63) == 0 && w_ < kTraceWaves / 2)                                  \
            g_trace[((A.t & 1u) * (kTraceWaves / 2) + w_) * 8 + (k)] = t_;                    \
    } while (0)
#else
#define TRACE_STAMP(k) \
    do {               \
    } while (0)
#endif

constexpr uint8_t kRecDone = 1, kRecInvalid = 2;  // replay ring flags byte (csrc/replay.h)

constexpr int64_t kRecMaxIters = 8;  // se_step_record's cut bits: 4 per group, <= 32 per thread

// se_step_record: the replay ring's end-of-step record (replay_end4_kernel's stores,
// csrc/replay.h) written by the step kernel from the state it holds in registers, and
// the cut envs restarted there (se_replay_end_reset). Null rew outside se_step_record.
struct StepRecord {
    float* rew;
    uint8_t* flags;
    uint32_t* n_pos;
    float* n_fuel;
    int64_t* d_size;
    int64_t head, cap, new_size;  // head, cap multiples of 4 (a group's slots are consecutive)
    uint8_t* cut;
    int32_t max_steps;
    uint32_t epoch;
};

struct StepArgs {
    const uint32_t* world;
    WorldDims dims;
    int64_t n;
    int64_t env_base;  // multiple of 4 (a quad of envs shares its draw blocks)
    uint64_t seed;
    uint32_t t;
    se_state st;
    const int32_t* act;   // agent index (kTyped = false) or type (kTyped = true)
    const int32_t* act_a;
    const int32_t* act_b;
    se_tape* tape;           // replay: variates in, used flags out
    se_done_rec* done_recs;  // this step's done list: per-(iteration, wave) segments of `seg` records
    int32_t* done_count;     // this step's per-segment record counts
    int64_t seg;             // segment stride (records) of one workgroup
    int32_t done_pad;        // done-list records padded to runs of this many (1: none; wave_compact)
    int64_t iters;           // groups per thread (each workgroup owns iters * 256 groups)
    double* slab;            // per-wave {sum_ret, n_eps, sum_len, pad}
    StepRecord rec;          // step_kernel<..., kRec = true> only
};

// The kernel's StepArgs re-read from the kernarg segment where a late phase needs
// them. The empty asm makes the compiler forget its SGPR copies, so pointers used
// only after the Philox / select stretch (store_rest, the episode counters, the done
// list, the slab) are fetched with s_load where they are used instead of staying
// live in SGPRs across it (the config-4 kernel spilled 44 SGPRs to VGPR lanes:
// ~135 v_writelane / v_readlane). StepArgs is the kernels' only argument, so it
// starts the kernarg segment.
typedef const __attribute__((address_space(4))) StepArgs* StepArgsK;
__device__ __forceinline__ const StepArgs& late_args() {
    StepArgsK p = (StepArgsK)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const StepArgs*)p;
}

// Field access for the 4 envs of one group. Full groups: the pointer advanced to
// the block-uniform first group g0 stays scalar and the lane offset is
// loop-invariant, so no per-access 64-bit address arithmetic runs on the VALU; each
// field is one 4-byte (u8 x4), 16-byte (32-bit x4) or 2 x 16-byte (f64 x4) lane
// access. The partial last group uses guarded scalar accesses at env index base.
template <typename T>
__device__ __forceinline__ T* slab_of(T* p, int64_t g0) {
    return p + g0 * 4;
}

// Streaming accesses: state is touched once per step, so stores carry the
// nontemporal hint (written lines do not linger dirty in L2 until the end-of-kernel
// writeback). Loads take it only when the step's working set is cache-resident
// (kNt, chosen per launch by step_nt_loads): measured faster at N = 2^20, slower
// at 2^24.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <bool kNt = false, typename V>
__device__ __forceinline__ V ld_stream(const V* p) {
    if constexpr (kNt) {
        if constexpr (sizeof(V) == 16)
            return __builtin_bit_cast(V, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)));
        else
            return __builtin_nontemporal_load(p);
    } else {
        return *p;
    }
}
template <typename V>
__device__ __forceinline__ void st_stream(V* p, V v) {
    if constexpr (sizeof(V) == 16)
        __builtin_nontemporal_store(__builtin_bit_cast(u32x4, v), reinterpret_cast<u32x4*>(p));
    else
        __builtin_nontemporal_store(v, p);
}

// the full-group stores: st_stream above at a byte offset
template <typename V>
__device__ __forceinline__ void st_at(void* base, uint32_t byte_off, V v) {
    st_stream(reinterpret_cast<V*>(reinterpret_cast<char*>(base) + byte_off), v);
}

template <bool kNt = false, typename T>
__device__ __forceinline__ void ld4_full(const T* __restrict__ p, int64_t g0, T (&v)[4],
                                         uint32_t lane = threadIdx.x) {
    if constexpr (sizeof(T) == 4) {
        const uint4 w = ld_stream<kNt>(reinterpret_cast<const uint4*>(slab_of(p, g0)) + lane);
        v[0] = __builtin_bit_cast(T, w.x);
        v[1] = __builtin_bit_cast(T, w.y);
        v[2] = __builtin_bit_cast(T, w.z);
        v[3] = __builtin_bit_cast(T, w.w);
    } else {
        const double2* q = reinterpret_cast<const double2*>(slab_of(p, g0)) + 2 * lane;
        const double2 a = ld_stream<kNt>(q), b = ld_stream<kNt>(q + 1);
        v[0] = a.x;
        v[1] = a.y;
        v[2] = b.x;
        v[3] = b.y;
    }
}

template <typename T>
__device__ __forceinline__ void st4_full(T* __restrict__ p, int64_t g0, const T (&v)[4],
                                         uint32_t lane = threadIdx.x) {
    if constexpr (sizeof(T) == 4) {
        uint4 w;
        w.x = __builtin_bit_cast(uint32_t, v[0]);
        w.y = __builtin_bit_cast(uint32_t, v[1]);
        w.z = __builtin_bit_cast(uint32_t, v[2]);
        w.w = __builtin_bit_cast(uint32_t, v[3]);
        st_at(slab_of(p, g0), 16u * lane, w);
    } else {
        st_at(slab_of(p, g0), 32u * lane, make_double2(v[0], v[1]));
        st_at(slab_of(p, g0), 32u * lane + 16u, make_double2(v[2], v[3]));
    }
}

template <typename T>
__device__ __forceinline__ void ld4_tail(const T* __restrict__ p, int64_t base, int64_t n, T (&v)[4]) {
    for (int j = 0; j < 4; ++j) v[j] = base + j < n ? p[base + j] : T(0);
}

template <typename T>
__device__ __forceinline__ void st4_tail(T* __restrict__ p, int64_t base, int64_t n, const T (&v)[4]) {
    for (int j = 0; j < 4; ++j)
        if (base + j < n) p[base + j] = v[j];
}

template <bool kNt = false>
__device__ __forceinline__ uint32_t ld4u8_full(const uint8_t* __restrict__ p, int64_t g0,
                                               uint32_t lane = threadIdx.x) {
    return ld_stream<kNt>(reinterpret_cast<const uint32_t*>(slab_of(p, g0)) + lane);
}
__device__ __forceinline__ void st4u8_full(uint8_t* __restrict__ p, int64_t g0, uint32_t w,
                                           uint32_t lane = threadIdx.x) {
    st_at(slab_of(p, g0), 4u * lane, w);
}
__device__ __forceinline__ uint32_t ld4u8_tail(const uint8_t* __restrict__ p, int64_t base, int64_t n) {
    uint32_t w = 0;
    for (int j = 0; j < 4; ++j)
        if (base + j < n) w |= (uint32_t)p[base + j] << (8 * j);
    return w;
}
__device__ __forceinline__ void st4u8_tail(uint8_t* __restrict__ p, int64_t base, int64_t n, uint32_t w) {
    for (int j = 0; j < 4; ++j)
        if (base + j < n) p[base + j] = (uint8_t)(w >> (8 * j));
}

__device__ __forceinline__ int byte_of(uint32_t w, int j) { return (int)((w >> (8 * j)) & 0xffu); }

// Where one group's fields live: g0 (block-uniform) for a full group, whose envs
// are 4 * (g0 + threadIdx.x) + j; base = the group's first env in both cases.
template <bool kFull>
struct At {
    int64_t g0, base, n;
};

// The inputs of the 4 envs of one group.
template <bool kTyped, bool kAuto, bool kNt = false>
struct Group {
    uint32_t x, y, org, dst;  // packed u8 x4
    int32_t c[4];             // cargo
    double f[4];              // fuel
    int32_t a[4];             // agent index / action type
    int32_t p[4], q[4];       // typed: values a, b
    float e[4];               // ep_return
    uint32_t l[4];            // ep_start: the step counter when the episode began

    // lane: the group within the block's row (threadIdx.x; the kernel's first load
    // clamps it into range instead of branching around the load)
    template <bool kFull>
    __device__ __forceinline__ void load(const StepArgs& A, At<kFull> at, uint32_t lane = threadIdx.x) {
        const se_state& S = A.st;
        if constexpr (kFull) {
            x = ld4u8_full<kNt>(S.x, at.g0, lane);
            y = ld4u8_full<kNt>(S.y, at.g0, lane);
            org = ld4u8_full<kNt>(S.origin, at.g0, lane);
            dst = ld4u8_full<kNt>(S.dest, at.g0, lane);
            ld4_full<kNt>(S.cargo, at.g0, c, lane);
            ld4_full<kNt>(S.fuel, at.g0, f, lane);
            ld4_full<kNt>(A.act, at.g0, a, lane);
            if (kTyped) {
                ld4_full<kNt>(A.act_a, at.g0, p, lane);
                ld4_full<kNt>(A.act_b, at.g0, q, lane);
            }
        } else {
            x = ld4u8_tail(S.x, at.base, at.n);
            y = ld4u8_tail(S.y, at.base, at.n);
            org = ld4u8_tail(S.origin, at.base, at.n);
            dst = ld4u8_tail(S.dest, at.base, at.n);
            ld4_tail(S.cargo, at.base, at.n, c);
            ld4_tail(S.fuel, at.base, at.n, f);
            ld4_tail(A.act, at.base, at.n, a);
            if (kTyped) {
                ld4_tail(A.act_a, at.base, at.n, p);
                ld4_tail(A.act_b, at.base, at.n, q);
            }
            if (kAuto) {
                ld4_tail(S.ep_return, at.base, at.n, e);
                ld4_tail(reinterpret_cast<const uint32_t*>(S.ep_start), at.base, at.n, l);
            }
        }
    }
    // episode counters of a full group, loaded late (step_group), where they would
    // otherwise hold 8 registers across the whole step: the running return of every
    // env, and the episode-start stamps only where they are needed, i.e. in the lanes
    // with an env that finishes in this step (`any`; about 1 env in 240 per step) or
    // for every env (kAll: se_step_record's max_steps cut). The stamps of other lanes
    // are never read or written, so a running length costs no traffic per step.
    template <bool kAll = false>
    __device__ __forceinline__ void load_episode(const StepArgs& A, At<true> at, bool any) {
        ld4_full<kNt>(A.st.ep_return, at.g0, e);
#pragma unroll
        for (int j = 0; j < 4; ++j) l[j] = 0u;
        if (kAll || any)
            ld4_full<kNt>(reinterpret_cast<const uint32_t*>(A.st.ep_start), at.g0, l);
    }
    template <bool kAll = false>
    __device__ __forceinline__ void load_episode(const StepArgs&, At<false>, bool) {}  // loaded with the rest
};

// Whether this lane's stamps move: one of its envs finished.
__device__ __forceinline__ bool stamp_lane(uint32_t fin) { return fin != 0; }

// ep_start of a group after a step at counter t: t + 1 for the envs that finished (the
// next step starts their new episode), unchanged for the others. A full group stores
// its lane's 16 bytes only when one of its envs finished; the partial last group
// stores its live envs.
template <bool kFull>
__device__ __forceinline__ void store_stamps(const se_state& S, At<kFull> at, const uint32_t (&l)[4],
                                             uint32_t fin, uint32_t t, bool any) {
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = ((fin >> j) & 1u) ? t + 1u : l[j];
    if constexpr (kFull) {
        if (any) st4_full(reinterpret_cast<uint32_t*>(S.ep_start), at.g0, v);
    } else {
        st4_tail(reinterpret_cast<uint32_t*>(S.ep_start), at.base, at.n, v);
    }
}

template <bool kFull, typename T>
__device__ __forceinline__ void store4(T* p, At<kFull> at, const T (&v)[4]) {
    if constexpr (kFull) st4_full(p, at.g0, v);
    else st4_tail(p, at.base, at.n, v);
}
template <bool kFull>
__device__ __forceinline__ void store4u8(uint8_t* p, At<kFull> at, uint32_t w) {
    if constexpr (kFull) st4u8_full(p, at.g0, w);
    else st4u8_tail(p, at.base, at.n, w);
}
