#pragma once
// world.h — the static world as every kernel sees it: the world image's layout
// (WorldDims), the exact small-integer helpers (mul24u, mul24i, sqrt_rn), the view
// of a staged image (LdsWorld, world_view) and its staging into LDS (stage_*).
//
// A fragment of shipenv.hip's translation unit, included inside its anonymous
// namespace where this text stood: not a stand-alone header. It is the first
// fragment and uses only shipenv.hip's own constants and include/shipenv.h.

// ------------------------------------------------------------------ world image
// One device buffer of 32-bit words, staged as-is into LDS by every workgroup:
//   [0, cw)         cell codes, one byte per cell c = x * W + y (x = map row, :65,
//                   :293): 0 water, kCellGround ground (np_game[x, y] == GROUND),
//                   k + 1 the FIRST port k on the cell (a port is never ground, :65;
//                   _get_current_port_idx returns the first match, :150-152).
//                   cw = H*W bytes rounded up to whole 16-byte units
//   [pos, +P)       port position  x | y << 16 (the packed form of a ship position)
//   [stk, +2P)      port stocks, (fuel, cargo) per port (8-byte aligned pairs)
//   [gate, +51)     u32 table floor(fl(c / 50) * 2^32) for c in [0, 50), and
//                   0xffffffff at 50: the gate on a Philox word (cargo >= 50 fires)
//   [frac, +100)    f64 table fl(c / 50) for c in [0, 50) (8-byte aligned; replay)
//   [rtab, +20)     f64 step rewards before cargo loss / arrival (8-byte aligned):
//                   [0, 8) a move, index out_of_fuel*4 + ground*2 + closer, summed in
//                   the reference's order (:288-315); [8] a take (0.05); [9] else 0
//   [moves, +4)     packed (dx, dy) of N, E, S, W (utils/preprocessing.py:126) as two
//                   16-bit halves: v_pk_add_u16 moves a packed position
// For the 100x100 map with 5 ports that is 10.8 KB: one byte lookup answers both
// "is the target cell ground" (:293) and "which port is the ship on" (:145-153),
// where bitmaps took a word read, bit arithmetic and a 3-read rank chain.
constexpr int kCellGround = 255;
// kStepBlock x 4-dword rows of the world image the step kernel stages unguarded
// (one 16-byte load per thread and row), at least 12 KB: the 100x100 image with up
// to 130 ports
constexpr int kStageRows = (3072 + 4 * kStepBlock - 1) / (4 * kStepBlock);
constexpr int kStageWords = kStageRows * 4 * kStepBlock;

struct WorldDims {
    int32_t H, W, P, cw;  // cw: words of cell codes (a multiple of 4)
    __host__ __device__ int pos() const { return cw; }
    __host__ __device__ int stk() const { return (pos() + P + 1) & ~1; }
    __host__ __device__ int gate() const { return stk() + 2 * P; }
    __host__ __device__ int frac() const { return (gate() + 51 + 1) & ~1; }
    __host__ __device__ int rtab() const { return frac() + 2 * 50; }
    __host__ __device__ int moves() const { return rtab() + 2 * 10; }
    __host__ __device__ int total() const { return moves() + 4; }
    // device image / LDS size: whole 1024-dword rows, at least the step kernel's
    // unguarded staging window
    __host__ __device__ int padded() const {
        const int t = (total() + 1023) / 1024 * 1024;
        return t > kStageWords ? t : kStageWords;
    }
};

// The per-env step core (env_begin / env_finish, the replayed step) is compiled for the
// host too: se_host_step_replay steps host-resident envs with the same source (the N = 1
// drop-in). The two helpers below are the only operations that differ between the
// targets; both are exact for the operand ranges used (< 2^24, correctly rounded sqrt).
__host__ __device__ inline uint32_t mul24u(uint32_t a, uint32_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umul24(a, b);
#else
    return a * b;
#endif
}
__host__ __device__ inline int mul24i(int a, int b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __mul24(a, b);
#else
    return a * b;
#endif
}
// IEEE square root, correctly rounded on both targets (np.sqrt, shipping/util.py:4)
__host__ __device__ inline double sqrt_rn(double v) {
#ifdef __HIP_DEVICE_COMPILE__
    return __dsqrt_rn(v);
#else
    return sqrt(v);
#endif
}

struct LdsWorld {
    const uint8_t* cell;
    const uint32_t* pos;
    const int2* stock;
    const uint32_t* gate_thr;
    const double* frac;
    const double* rtab;
    const uint32_t* moves;
    int32_t H, W, P;

    // cell index x * W + y: coordinates and W are below 256, so 24-bit multiplies
    // (full rate) are exact where a 32-bit one would be a 64-bit-product op
    __host__ __device__ int code(int x, int y) const { return cell[mul24u((uint32_t)x, (uint32_t)W) + (uint32_t)y]; }
    __host__ __device__ bool is_ground(int x, int y) const { return code(x, y) == kCellGround; }
    // _get_current_port_idx (:145-153): first port on the ship's cell, -1 if none
    // (water 0 -> -1, ground 255 -> 254 >= P)
    __host__ __device__ int port_at(int x, int y) const { return port_of_code(code(x, y)); }
    __host__ __device__ int port_of_code(int c) const {
        const int k = c - 1;
        return (unsigned)k < (unsigned)P ? k : -1;
    }
    __host__ __device__ int px(int i) const { return (int)(pos[i] & 0xffffu); }
    __host__ __device__ int py(int i) const { return (int)(pos[i] >> 16); }
    __host__ __device__ int pfuel(int i) const { return stock[i].x; }
    __host__ __device__ int pcargo(int i) const { return stock[i].y; }
    // normalize(cargo, 50, 0) (util.py:6-8), only read for 0 < cargo < 50
    __host__ __device__ double likelihood(int cargo) const { return frac[cargo]; }
};

__host__ __device__ inline LdsWorld world_view(WorldDims d, const uint32_t* img) {
    LdsWorld w;
    w.cell = reinterpret_cast<const uint8_t*>(img);
    w.pos = img + d.pos();
    w.stock = reinterpret_cast<const int2*>(img + d.stk());
    w.gate_thr = img + d.gate();
    w.frac = reinterpret_cast<const double*>(img + d.frac());
    w.rtab = reinterpret_cast<const double*>(img + d.rtab());
    w.moves = img + d.moves();
    w.H = d.H;
    w.W = d.W;
    w.P = d.P;
    return w;
}

// Staging in two halves. stage_issue puts every thread's share of the image in
// flight at once (independent 16-byte loads into registers); stage_finish writes it
// to LDS and holds the barrier. A load -> wait -> ds_write loop would make each
// round a full L2 round trip behind whatever the wave loaded before it (its
// s_waitcnt vmcnt(0) also waits for those). The step kernel issues its first
// group's loads between the halves, so the image (first in the in-order vmcnt
// queue) is written while the group's data is still on its way.
struct Staged {
    uint4 r[kStageRows];
};

// The step kernel's half (kStepBlock threads): the image is padded to at least
// kStageWords (WorldDims::padded), so these loads need no guard and no branch.
__device__ __forceinline__ Staged stage_issue(const uint32_t* __restrict__ g) {
    Staged st;
    const uint4* g4 = reinterpret_cast<const uint4*>(g);
#pragma unroll
    for (int k = 0; k < kStageRows; ++k) st.r[k] = g4[threadIdx.x + kStepBlock * k];
    return st;
}

__device__ __forceinline__ void stage_write(const uint32_t* __restrict__ g, WorldDims d, uint32_t* lds,
                                            const Staged& st) {
    uint4* l4 = reinterpret_cast<uint4*>(lds);
#pragma unroll
    for (int k = 0; k < kStageRows; ++k) l4[threadIdx.x + kStepBlock * k] = st.r[k];
    for (int i = (int)threadIdx.x + kStepBlock * kStageRows; i < (d.total() + 3) / 4; i += kStepBlock)
        l4[i] = reinterpret_cast<const uint4*>(g)[i];  // larger maps / port tables: the remainder
}
__device__ __forceinline__ LdsWorld stage_finish(const uint32_t* __restrict__ g, WorldDims d,
                                                 uint32_t* lds, const Staged& st) {
    stage_write(g, d, lds, st);
    __syncthreads();
    return world_view(d, lds);
}

// Any block size (the other kernels): every thread's 16-byte loads issued before any
// store (the image is padded to whole 1024-dword rows).
__device__ __forceinline__ LdsWorld stage_world(const uint32_t* __restrict__ g, WorldDims d,
                                                uint32_t* lds) {
    const int total = (d.total() + 3) / 4;
    const uint4* g4 = reinterpret_cast<const uint4*>(g);
    uint4* l4 = reinterpret_cast<uint4*>(lds);
    constexpr int kR = 4;
    for (int i0 = 0; i0 < total; i0 += kR * (int)blockDim.x) {
        // unconditional loads (past the end: the last word again), so r stays in VGPRs: a
        // conditionally assigned array was placed in scratch
        uint4 r[kR];
#pragma unroll
        for (int k = 0; k < kR; ++k) r[k] = g4[min(i0 + (int)threadIdx.x + k * (int)blockDim.x, total - 1)];
#pragma unroll
        for (int k = 0; k < kR; ++k) {
            const int i = i0 + (int)threadIdx.x + k * (int)blockDim.x;
            if (i < total) l4[i] = r[k];
        }
    }
    __syncthreads();
    return world_view(d, lds);
}
